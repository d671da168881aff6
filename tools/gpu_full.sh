#!/bin/bash
# One GPU call: parity tests, smoke, bench (c3 with both trust-region rules and the CPU baseline: --full; c2 the same;
# c4; c5), rocprof kernel stats.  Logs go to $OUT (default bench_logs/).
# Each GPU step time-limited;
# a crash / timeout (anything but pytest's "tests failed" rc 1) ends the script.
# usage: [OUT=dir] tools/gpu_full.sh TAG [pytest-args...]
set -e
export TMPDIR=/tmp
OUT=${OUT:-bench_logs}
mkdir -p $OUT
TAG=${1:-r2}
shift || true
timeout -k 10 700 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread "$@" > $OUT/pytest_gpu_$TAG.log 2>&1 || { rc=$?; echo "pytest rc $rc"; [ $rc -eq 1 ] || exit $rc; }
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1
timeout -k 10 300 python -u bench.py --full > $OUT/bench_$TAG.log 2>&1
timeout -k 10 300 python -u bench.py --full --config c2 > $OUT/bench_c2_$TAG.log 2>&1
timeout -k 10 300 python -u bench.py --config c4 > $OUT/bench_c4_$TAG.log 2>&1
timeout -k 10 300 python -u bench.py --config c5 > $OUT/bench_c5_$TAG.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python3 -u bench.py --steps 10 --warmup 3 > $OUT/bench_prof_$TAG.log 2>&1
timeout -k 10 60 rocprofv3 -L > $OUT/counters_list.txt 2>&1 || true
echo done
