#!/bin/bash
# The table of DESIGN.md 4.18 in one visit: tools/cmdref_profile.py under rocprofv3 --kernel-trace --stats, one scalar type per process (no counters in
# these runs): cmd_reference_kernel and cmd_swing_reference_kernel beside com_reference_kernel and com_swing_reference_kernel of the same build on the
# same states, 35 launches each.  Every step has its own time limit and the first failure ends the visit.
# usage (on the GPU box, from the repository root): bash tools/cmdref_profile.sh <output dir>
#        the log is <output dir>/cmdref_profile.log: per run the first rows of rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, AverageNs, ...)
set -u -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:?output dir}"
mkdir -p "$O"
LOG="$O/cmdref_profile.log"
: > "$LOG"
run() {   # run <dtype>
  local dt="$1" tag="cmdref_$1"
  echo "== $tag: cmdref_profile.py $dt" >> "$LOG"
  timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O" -o "$tag" -- python3 "$R/tools/cmdref_profile.py" "$dt" >> "$LOG" 2>> "$O/rocprof.err" || return 1
  local f
  f="$(find "$O" -name "${tag}_kernel_stats.csv" | head -1)"
  [ -n "$f" ] || { echo "no kernel statistics for $tag" >> "$LOG"; return 1; }
  head -7 "$f" >> "$LOG"
}
run f64 && run f32 || exit 1
echo "== done" >> "$LOG"
