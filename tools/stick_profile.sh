#!/bin/bash
# The timing table of DESIGN.md 4.13 in one visit: tools/stick_profile.py under rocprofv3 --kernel-trace --stats, one scalar type per process (no
# counters in these runs): stick_integrate_kernel, stick_force_kernel and, as the yardstick, ground_integrate_kernel of the same build, launched in
# turn on the same 4 096 states.  Every step has its own time limit and the first failure ends the visit.
# usage (on the GPU box, from the repository root): bash tools/stick_profile.sh <output dir>
#        the log is <output dir>/stick_profile.log: per run the first rows of rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, AverageNs, ...)
set -u -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:?output dir}"
mkdir -p "$O"
LOG="$O/stick_profile.log"
: > "$LOG"
run() {   # run <dtype>
  local dt="$1" tag="stick_$1"
  echo "== $tag: stick_profile.py $dt" >> "$LOG"
  timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O" -o "$tag" -- python3 "$R/tools/stick_profile.py" "$dt" >> "$LOG" 2>> "$O/rocprof.err" || return 1
  local f
  f="$(find "$O" -name "${tag}_kernel_stats.csv" | head -1)"
  [ -n "$f" ] || { echo "no kernel statistics for $tag" >> "$LOG"; return 1; }
  grep -E "^\"?Name|stick_|ground_integrate" "$f" >> "$LOG"
}
run f64 && run f32 || exit 1
echo "== done" >> "$LOG"
