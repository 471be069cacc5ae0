#!/bin/bash
# The table of DESIGN.md 4.12 in one visit: tools/ground_profile.py under rocprofv3 --kernel-trace --stats, one phase and scalar type per process (no
# counters in these runs): ground_integrate_kernel, ground_force_kernel + integrate_kernel, and -- when given -- integrate_kernel of the build before
# the ground entry points as the yardstick (else this build's, which is the same code).  Every step has its own time limit and the first failure ends
# the visit.
# usage (on the GPU box, from the repository root): bash tools/ground_profile.sh <output dir> [libwbc_hip.so of the parent commit]
#        the log is <output dir>/ground_profile.log: per run the first rows of rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, AverageNs, ...)
set -u -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:?output dir}"
PARENT="${2:-}"
mkdir -p "$O"
LOG="$O/ground_profile.log"
: > "$LOG"
run() {   # run <tag> <library or ""> <phase> <dtype>
  local tag="$1" libso="$2" phase="$3" dt="$4"
  echo "== $tag: ground_profile.py $phase $dt ${libso:+(WBC_LIB=$libso)}" >> "$LOG"
  ( [ -n "$libso" ] && export WBC_LIB="$libso"
    timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O" -o "$tag" -- python3 "$R/tools/ground_profile.py" "$phase" "$dt" ) >> "$LOG" 2>> "$O/rocprof.err" || return 1
  local f
  f="$(find "$O" -name "${tag}_kernel_stats.csv" | head -1)"
  [ -n "$f" ] || { echo "no kernel statistics for $tag" >> "$LOG"; return 1; }
  head -8 "$f" >> "$LOG"
}
for dt in f64 f32; do
  run "fused_$dt" "" fused "$dt" && run "two_$dt" "" two "$dt" && run "integrate_$dt" "$PARENT" integrate "$dt" || exit 1
done
echo "== done" >> "$LOG"
