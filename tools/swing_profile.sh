#!/bin/bash
# The table of DESIGN.md 4.10 in one visit: tools/swing_profile.py under rocprofv3 --kernel-trace --stats, one phase and scalar type per process (no
# counters in these runs): the stand-alone swing kernel, the fused kernel, and com_reference_kernel of this build and -- when given -- of the build
# before the swing entry points as the yardstick.  Every step has its own time limit and the first failure ends the visit.
# usage (on the GPU box, from the repository root): bash tools/swing_profile.sh <output dir> [libwbc_hip.so of the parent commit]
#        the log is <output dir>/swing_profile.log: per run the first rows of rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, AverageNs, ...)
set -u -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:?output dir}"
PARENT="${2:-}"
mkdir -p "$O"
LOG="$O/swing_profile.log"
: > "$LOG"
run() {   # run <tag> <library or ""> <phase> <dtype>
  local tag="$1" libso="$2" phase="$3" dt="$4"
  echo "== $tag: swing_profile.py $phase $dt ${libso:+(WBC_LIB=$libso)}" >> "$LOG"
  ( [ -n "$libso" ] && export WBC_LIB="$libso"
    timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O" -o "$tag" -- python3 "$R/tools/swing_profile.py" "$phase" "$dt" ) >> "$LOG" 2>> "$O/rocprof.err" || return 1
  local f
  f="$(find "$O" -name "${tag}_kernel_stats.csv" | head -1)"
  [ -n "$f" ] || { echo "no kernel statistics for $tag" >> "$LOG"; return 1; }
  head -6 "$f" >> "$LOG"
}
for dt in f64 f32; do
  run "swing_$dt" "" swing "$dt" && run "fused_$dt" "" fused "$dt" && run "ref_$dt" "" ref "$dt" || exit 1
  if [ -n "$PARENT" ]; then run "ref_parent_$dt" "$PARENT" ref "$dt" || exit 1; fi
done
echo "== done" >> "$LOG"
