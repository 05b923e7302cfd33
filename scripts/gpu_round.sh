#!/bin/bash
# One GPU-box session: parity tests, bench, rocprofv3 kernel trace. Stops at the first fault/timeout.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}   # where this session's files go
mkdir -p $OUT
export TMPDIR=/tmp
ok() { [ "$1" -eq 0 ]; }
if [ "${SKIP_TESTS:-0}" != 1 ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -v --timeout 120 --timeout-method thread \
      > $OUT/pytest_gpu.log 2>&1
  rc=$?; echo "PYTEST rc=$rc"; grep -E "passed|failed" $OUT/pytest_gpu.log | tail -2
  grep -E "FAILED|Error" $OUT/pytest_gpu.log | head -20
  ok $rc || exit $rc
fi
timeout -k 10 400 python -u bench.py --full ${BENCH_ARGS:-} > $OUT/bench.json 2> $OUT/bench.err
rc=$?; echo "BENCH rc=$rc"; cat $OUT/bench.json; tail -5 $OUT/bench.err
[ $rc -eq 0 ] || exit $rc
if [ "${SKIP_PROF:-0}" != 1 ]; then
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$PWD/$OUT/prof" -o bench -- \
      python -u bench.py --steps 5 --warmup 1 --no-cpu-baseline > $OUT/prof.log 2>&1
  rc=$?; echo "PROF rc=$rc"; tail -3 $OUT/prof.log
  find $OUT/prof -name "*stats*" | head
fi
