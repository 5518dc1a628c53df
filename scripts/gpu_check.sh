#!/bin/bash
# Runs on the GPU box: smoke -> pytest -m gpu -> bench.py --full -> rocprofv3 kernel stats of the bench.
# Every step runs under timeout and the script stops at the first one that fails; outputs land in $OUT (default: check_out/).
cd "$(dirname "$0")/.."
R=$PWD
mkdir -p "${OUT:-check_out}" && O=$(cd "${OUT:-check_out}" && pwd) || exit 1
export TMPDIR=/tmp
rocm-smi --showproductname 2>/dev/null | head -8 > "$O/gpu.txt"
nproc >> "$O/gpu.txt"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1; rc=$?; echo "smoke rc=$rc"
tail -3 "$O/smoke.log"; [ $rc -eq 0 ] || exit $rc
if [ "${SKIP_TESTS:-0}" != "1" ]; then
timeout -k 10 900 python -m pytest tests -x -q -m gpu --durations=12 > "$O/pytest_gpu.log" 2>&1; rc=$?; echo "pytest rc=$rc"
tail -25 "$O/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 600 python bench.py --full --steps ${STEPS:-20} --warmup 3 > "$O/bench.json" 2> "$O/bench.err"; rc=$?; echo "bench rc=$rc"
cat "$O/bench.json"; tail -5 "$O/bench.err"; [ $rc -eq 0 ] || exit $rc
if [ "${SKIP_PROF:-0}" != "1" ]; then
cd /tmp
rm -rf "$O/prof"
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$O/prof" -o bench -- python "$R/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline --no-e2e > "$O/bench_prof.json" 2> "$O/prof.err"; rc=$?; echo "rocprof rc=$rc"
cd "$R"
find "$O/prof" -name "*stats*" | head
for f in $(find "$O/prof" -name "*kernel_stats.csv"); do head -12 "$f"; done
# keep the payload small: drop the raw per-dispatch trace, keep the stats
find "$O/prof" -name "*kernel_trace.csv" -size +20M -delete
exit $rc
fi
