#!/bin/bash
# GPU check: tests -> smoke -> short bench. Stops at the first crash/timeout (rc not in {0,1}).
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p gpurun_out
timeout -k 10 900 python -m pytest tests -q -m gpu --timeout 300 -x > gpurun_out/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -5 gpurun_out/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -3 gpurun_out/smoke.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
# a --full run: the short bench with its side measurements (CPU baseline included)
BENCH_ARGS="--full ${BENCH_ARGS:---games 8192 --steps 2 --warmup 1 --cpu-seconds 10}"
timeout -k 10 600 python bench.py ${BENCH_ARGS:---games 8192 --steps 2 --warmup 1 --cpu-seconds 10} > gpurun_out/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -3 gpurun_out/bench.log
exit $rc
