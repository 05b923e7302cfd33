#!/bin/bash
# One profiling session on the GPU box: the default bench line, a rocprofv3 kernel trace (--stats), and two
# PMC passes (FETCH_SIZE, WRITE_SIZE: they cannot share a pass) over a short bench run. Stops at the first
# failure. Outputs under $OUT/ (copy the summaries into profiles/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}   # where this session's files go
mkdir -p $OUT
export TMPDIR=/tmp
rm -rf $OUT/prof $OUT/pmc_fetch $OUT/pmc_write
timeout -k 10 400 python -u bench.py --full ${BENCH_ARGS:-} > $OUT/bench.json 2> $OUT/bench.err
rc=$?; echo "BENCH rc=$rc"; cat $OUT/bench.json; tail -3 $OUT/bench.err
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$PWD/$OUT/prof" -o bench --output-format csv -- \
    python -u bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-extras ${BENCH_ARGS:-} > $OUT/prof.log 2>&1
rc=$?; echo "PROF rc=$rc"; tail -2 $OUT/prof.log
[ $rc -eq 0 ] || exit $rc
for ctr in FETCH_SIZE WRITE_SIZE; do
  d=$OUT/pmc_$(echo $ctr | tr A-Z a-z | cut -d_ -f1)
  timeout -s KILL 240 rocprofv3 --pmc $ctr -d "$PWD/$d" -o pmc --output-format csv -- \
      python -u bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-extras ${BENCH_ARGS:-} > $d.log 2>&1
  rc=$?; echo "PMC $ctr rc=$rc"; tail -2 $d.log
  [ $rc -eq 0 ] || exit $rc
done
find $OUT/prof $OUT/pmc_* -name "*.csv" | head -20
python scripts/pmc_summary.py $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_latest.json
