#!/bin/bash
# The table of DESIGN.md 4.16 in one visit: tools/foothold_profile.py under rocprofv3 --kernel-trace --stats, one scalar type and one ground per process
# (no counters in these runs): gait_terrain_select_kernel and gait_estimated_terrain_select_kernel beside gait_terrain_kernel and
# gait_estimated_terrain_kernel of the same build on the same states, foothold_select_kernel and terrain_cost_kernel, 35 launches each.
# Every step has its own time limit and the first failure ends the visit.
# usage (on the GPU box, from the repository root): bash tools/foothold_profile.sh <output dir>
#        the log is <output dir>/foothold_profile.log: per run the first rows of rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, AverageNs, ...)
set -u -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:?output dir}"
mkdir -p "$O"
LOG="$O/foothold_profile.log"
: > "$LOG"
run() {   # run <dtype> <ground>
  local dt="$1" gr="$2" tag="foothold_$1_$2"
  echo "== $tag: foothold_profile.py $dt $gr" >> "$LOG"
  timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O" -o "$tag" -- python3 "$R/tools/foothold_profile.py" "$dt" "$gr" >> "$LOG" 2>> "$O/rocprof.err" || return 1
  local f
  f="$(find "$O" -name "${tag}_kernel_stats.csv" | head -1)"
  [ -n "$f" ] || { echo "no kernel statistics for $tag" >> "$LOG"; return 1; }
  head -10 "$f" >> "$LOG"
}
run f64 quiet && run f64 ridges && run f32 quiet && run f32 ridges || exit 1
echo "== done" >> "$LOG"
