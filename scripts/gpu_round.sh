#!/bin/bash
# One GPU round trip: the full -m gpu suite (one pytest process), then the default bench with its
# CPU leg and parity block (bench.py --full). Each GPU step has its own time limit; a failed step
# ends the script. Usage: OUT=dir gpu_round.sh [TAG]
export TMPDIR=/tmp
TAG=${1:-run}
OUT=${OUT:?set OUT to the output directory}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread -p no:cacheprovider -rP \
  --tb=short > $OUT/pytest_gpu_$TAG.log 2>&1
rc=$?
echo "pytest exit $rc" >> $OUT/pytest_gpu_$TAG.log
grep -E "passed|failed|error" $OUT/pytest_gpu_$TAG.log | tail -5
[ $rc -le 1 ] || exit $rc
timeout -k 10 600 python -u bench.py --full --json-out $OUT/bench_$TAG.json > $OUT/bench_$TAG.log 2>&1
rc2=$?
echo "bench exit $rc2"; tail -c 600 $OUT/bench_$TAG.log
exit $(( rc > rc2 ? rc : rc2 ))
