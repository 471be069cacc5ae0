#!/bin/bash
# The table of DESIGN.md 4.14 in one visit: tools/contact_profile.py under rocprofv3 --kernel-trace --stats, one phase and scalar type per process (no
# counters in these runs): contact_estimate_kernel, gait_estimated_kernel and, as the yardstick, gait_kernel of the same build on the same states.
# Every step has its own time limit and the first failure ends the visit.
# usage (on the GPU box, from the repository root): bash tools/contact_profile.sh <output dir>
#        the log is <output dir>/contact_profile.log: per run the first rows of rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, AverageNs, ...)
set -u -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:?output dir}"
mkdir -p "$O"
LOG="$O/contact_profile.log"
: > "$LOG"
run() {   # run <phase> <dtype>
  local phase="$1" dt="$2" tag="$1_$2"
  echo "== $tag: contact_profile.py $phase $dt" >> "$LOG"
  timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O" -o "$tag" -- python3 "$R/tools/contact_profile.py" "$phase" "$dt" >> "$LOG" 2>> "$O/rocprof.err" || return 1
  local f
  f="$(find "$O" -name "${tag}_kernel_stats.csv" | head -1)"
  [ -n "$f" ] || { echo "no kernel statistics for $tag" >> "$LOG"; return 1; }
  head -6 "$f" >> "$LOG"
}
for dt in f64 f32; do
  run estimate "$dt" && run fused "$dt" && run gait "$dt" || exit 1
done
echo "== done" >> "$LOG"
