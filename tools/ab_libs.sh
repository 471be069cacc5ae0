#!/bin/bash
# A/B of library builds on one device (directories under wbc_quadruped_dob_amd/, e.g. lib lib_variant; a variant is built with
#   make -C wbc_quadruped_dob_amd/csrc -j8 LIBDIR=../lib_variant EXTRA=-DSOME_MACRO=1 ).  Replaces round 4's one-off r04_*.sh scripts.
#   tools/ab_libs.sh "<bench args>" libA libB ...          bench.py lines: steps/s, ms per step, the tick's kernels; with --closed-loop the cold / warm loop,
#                                                           with --config 5 the rollout's time per tick
#   tools/ab_libs.sh loops "<sizes>" libA libB ...         tools/warm_loop.py with WARM_LOOP_LANE=1: cold / warm without the per-lane pair / warm per-lane pair / warm
#                                                           one-wavefront kernel forced, per size and workload
#   tools/ab_libs.sh tests "<pytest args>" libA ...        the GPU tests against a library build
#   tools/ab_libs.sh plain "<bench args>" libA libB ...    the PLAIN bench.py run (what the headline is), builds alternating, REPS (default 5) runs each; then
#                                                           median and min - max of `value` per build, and the gain rule (first item): it is a gain only
#                                                           if the two ranges do not overlap and the median gain is at least three times the first build's own
#                                                           min - max spread.  What bench.py writes to stderr is kept in ab_libs_plain.err beside the working directory's
#                                                           other output (AB_ERR to put it elsewhere)
set -u
export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT:-/root/repo}"
what="$1"; shift
if [ "$what" = "loops" ]; then
  sizes="$1"; shift
  for L in "$@"; do
    echo "== $L"
    WBC_LIB=$PWD/wbc_quadruped_dob_amd/$L/libwbc_hip.so WARM_LOOP_LANE=1 timeout 1500 python tools/warm_loop.py $sizes 2>/dev/null
  done
  exit 0
fi
if [ "$what" = "plain" ]; then
  pargs="$1"; shift
  vals=$(mktemp); trap 'rm -f "$vals"' EXIT
  err=${AB_ERR:-$PWD/ab_libs_plain.err}; : > "$err"
  for rep in $(seq 1 ${REPS:-5}); do for L in "$@"; do
    v=$(WBC_LIB=$PWD/wbc_quadruped_dob_amd/$L/libwbc_hip.so timeout -k 10 300 python bench.py $pargs 2>> "$err" | python -c 'import sys, json; print("%.3f" % (json.loads(sys.stdin.read())["value"] / 1e6))') || { echo "bench.py failed: $L rep $rep (stderr: $err)"; tail -5 "$err"; exit 1; }
    echo "$L [$pargs] rep $rep  $v M/s"; echo "$L $v" >> $vals
  done; done
  python - $vals "$@" <<'PY'
import sys, statistics
rows = [l.split() for l in open(sys.argv[1])]
base = None
for L in sys.argv[2:]:
    v = sorted(float(x) for n, x in rows if n == L)
    med = statistics.median(v)
    line = "%-24s median %8.2f M/s   min - max %8.2f - %8.2f (spread %.2f)" % (L, med, v[0], v[-1], v[-1] - v[0])
    if base is None: base = (med, v[0], v[-1])
    else: line += "   vs %s: %+.2f %%, ranges %s, gain / its spread %.1f" % (sys.argv[2], 100 * (med / base[0] - 1), "overlap" if v[0] <= base[2] and base[1] <= v[-1] else "apart", (med - base[0]) / max(base[2] - base[1], 1e-9))
    print(line)
PY
  exit 0
fi
if [ "$what" = "tests" ]; then
  targs="$1"; shift
  for L in "$@"; do
    echo "== $L"
    WBC_LIB=$PWD/wbc_quadruped_dob_amd/$L/libwbc_hip.so timeout 1500 python -m pytest $targs -q 2>&1 | grep -E "passed|failed|^E " | tail -8
  done
  exit 0
fi
args="$what"
pick='
import sys, json
d = json.loads(sys.stdin.read()); k = d.get("kernels") or {}
f = lambda x: "-" if x is None else "%.1f" % x
line = "%-44s %8.1f M/s %8.4f ms/step" % (sys.argv[1], d["value"] / 1e6, d["ms_per_step"])
if "us_per_tick" in d: line += "  %.2f us/tick" % d["us_per_tick"]
if k: line += "  fused %s sweep %s front2 %s qp %s lane %s" % tuple(f(k.get(x)) for x in ("fused_tick_us", "dyn_sweep_us", "rnea_step_us", "qp_us", "qp_lane_us"))
c = d.get("closed_loop")
if c and "cold" in c: line += "  | closed loop cold %.2f us (kernels %.1f) warm %.2f us (kernels %.1f)" % (c["cold"]["us_per_tick"], c["cold"]["kernels_sum_us"], c["warm"]["us_per_tick"], c["warm"]["kernels_sum_us"])
print(line)'
for rep in 1 2 3; do for L in "$@"; do
  WBC_LIB=$PWD/wbc_quadruped_dob_amd/$L/libwbc_hip.so python bench.py --full --no-cpu --no-latency --large-batch 0 $args 2>/dev/null | python -c "$pick" "$L [$args] rep $rep"
done; done
