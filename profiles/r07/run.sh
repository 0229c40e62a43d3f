#!/bin/bash
# new tests, smoke, probe under rocprofv3 kernel trace, bench; every GPU step under its own time limit, stop at the first failure
set -u
rm -rf out/r07; mkdir -p out/r07
export PYTHONDONTWRITEBYTECODE=1
timeout -k 10 1200 python -m pytest -q -p no:cacheprovider tests/test_full_softmax_gpu.py > out/r07/gpu_tests.txt 2>&1; rc=$?
tail -5 out/r07/gpu_tests.txt; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" > out/r07/smoke.txt 2>&1; rc=$?
tail -1 out/r07/smoke.txt; [ $rc -eq 0 ] || exit $rc
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d out/r07/rocprof -o probe -- python tools/full_softmax_probe.py --reps 3 --out out/r07/full_softmax_probe.txt > out/r07/probe_log.txt 2>&1; rc=$?
[ $rc -eq 0 ] || { tail -30 out/r07/probe_log.txt; exit $rc; }
cat out/r07/full_softmax_probe.txt; find out/r07/rocprof -name "*stats*"
timeout -k 10 900 python bench.py --gpus 1 --steps 20 --warmup 5 > out/r07/bench.txt 2>&1; rc=$?
tail -1 out/r07/bench.txt | cut -c1-300; exit $rc
