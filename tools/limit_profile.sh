#!/bin/bash
# The table of DESIGN.md 4.9 in one visit: tools/limit_profile.py under rocprofv3 --kernel-trace --stats, one phase per process (no counters in
# these runs), the plain tick of this build and of the build before the post-pass alternating three times each (the run-to-run spread the comparison
# is read against), then tools/bw_probe.bin on the scan's footprint (13 rows read, 1 written).  Every step has its own time limit and the first
# failure ends the visit.
# usage (on the GPU box, from the repository root): bash tools/limit_profile.sh <output dir> [libwbc_hip.so of the parent commit]
#        the log is <output dir>/limit_profile.log: per run the first rows of rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, AverageNs, Percentage, MinNs, MaxNs, StdDev)
set -u -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:?output dir}"
PARENT="${2:-}"
mkdir -p "$O"
LOG="$O/limit_profile.log"
: > "$LOG"
run() {   # run <tag> <library or ""> <phase>
  local tag="$1" libso="$2" phase="$3"
  echo "== $tag: limit_profile.py $phase ${libso:+(WBC_LIB=$(basename "$(dirname "$libso")")/$(basename "$libso"))}" >> "$LOG"
  ( [ -n "$libso" ] && export WBC_LIB="$libso"
    timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O" -o "$tag" -- python3 "$R/tools/limit_profile.py" "$phase" ) >> "$LOG" 2>> "$O/rocprof.err" || return 1
  local f
  f="$(find "$O" -name "${tag}_kernel_stats.csv" | head -1)"
  [ -n "$f" ] || { echo "no kernel statistics for $tag" >> "$LOG"; return 1; }
  head -12 "$f" >> "$LOG"
}
for rep in 1 2 3; do
  run "tick_this_$rep" "" tick || exit 1
  if [ -n "$PARENT" ]; then run "tick_parent_$rep" "$PARENT" tick || exit 1; fi
done
run limit_inf "" inf && run limit_60 "" 60 && run limit_8 "" 8 && run limit_60_again "" 60 && run limit_8_again "" 8 || exit 1
echo "== bw_probe.bin rw 8 13 1 4096 (GB/s, us per launch: back-to-back launches between two events)" >> "$LOG"
timeout -k 10 60 "$R/tools/bw_probe.bin" rw 8 13 1 4096 >> "$LOG" 2>&1 || exit 1
echo "== done" >> "$LOG"
