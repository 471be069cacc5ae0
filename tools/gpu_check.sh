#!/bin/bash
# Runs on a machine with the GPU: GPU parity tests, smoke, bench --full (default, bare --gpus 2, single-process 2 shards), rocprof.
# usage: tools/gpu_check.sh [output directory, default gpu_check_out/ in the repository root]
set -u
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:-$R/gpu_check_out}"
mkdir -p "$O" && O="$(cd "$O" && pwd)"
cd "$R"
export TMPDIR=/tmp
python -m pytest tests -x -q -m gpu 2>&1 | tail -25 > "$O/pytest_gpu.log"
echo "pytest exit: ${PIPESTATUS[0]}" >> "$O/pytest_gpu.log"
python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1
echo "smoke exit: $?" >> "$O/smoke.log"
python bench.py --full --steps 20 --warmup 5 > "$O/bench.json" 2> "$O/bench.err"
echo "bench exit: $?" >> "$O/bench.err"
python bench.py --full --gpus 2 --steps 20 --warmup 5 > "$O/bench_gpus2.json" 2> "$O/bench_gpus2.err"
echo "bench --gpus 2 exit: $?" >> "$O/bench_gpus2.err"
python bench.py --full --gpus 2 --single-process --steps 20 --warmup 5 > "$O/bench_sp2.json" 2> "$O/bench_sp2.err"
echo "bench --gpus 2 --single-process exit: $?" >> "$O/bench_sp2.err"
python bench.py --full --steps 50 --warmup 5 --batch 262144 --no-cpu --no-latency --large-batch 0 > "$O/bench_262144.json" 2>> "$O/bench.err"
if [ "${PROFILE:-1}" = "1" ]; then
  rm -rf "$O/prof" && mkdir -p "$O/prof"
  ( cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -o r02 -- python3 "$R/bench.py" --full --steps 200 --warmup 20 --no-cpu --no-latency --large-batch 0 > "$O/prof/bench_under_rocprof.json" 2> "$O/prof/rocprof.err" )
  find "$O/prof" -name "*kernel_trace.csv" -size +2M -delete
fi
cat "$O/pytest_gpu.log" "$O/smoke.log" "$O/bench.json" "$O/bench_gpus2.err" "$O/bench_sp2.json" "$O/bench_sp2.err" "$O/bench_262144.json"
tail -5 "$O/bench.err"
