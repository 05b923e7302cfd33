#!/bin/bash
# Round-5 measurement session: PMC passes first (the bench line reads profiles/pmc_latest.json for its traffic field),
# the default bench line (CPU baseline included), a kernel trace (--stats), the commit-kernel stamps, smoke(), and
# the C5 bench at 100k nodes. Each step under its own limit; stops at the first failure.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}   # where this session's files go
mkdir -p $OUT
export TMPDIR=/tmp
rm -rf $OUT/prof $OUT/pmc_fetch $OUT/pmc_write
for ctr in FETCH_SIZE WRITE_SIZE; do
  d=$OUT/pmc_$(echo $ctr | tr A-Z a-z | cut -d_ -f1)
  timeout -s KILL 240 rocprofv3 --pmc $ctr -d "$PWD/$d" -o pmc --output-format csv -- \
      python -u bench.py --steps 1 --warmup 0 --no-cpu-baseline > $d.log 2>&1
  rc=$?; echo "PMC $ctr rc=$rc"; tail -2 $d.log
  [ $rc -eq 0 ] || exit $rc
done
python scripts/pmc_summary.py $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_latest.json || exit 1
cp $OUT/pmc_latest.json profiles/pmc_latest.json
timeout -k 10 500 python -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err
rc=$?; echo "BENCH rc=$rc"; cat $OUT/bench.json; tail -3 $OUT/bench.err
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$PWD/$OUT/prof" -o bench --output-format csv -- \
    python -u bench.py --steps 5 --warmup 1 --no-cpu-baseline > $OUT/prof.log 2>&1
rc=$?; echo "PROF rc=$rc"; tail -2 $OUT/prof.log
[ $rc -eq 0 ] || exit $rc
GS_COMMIT_STAMPS=1 timeout -k 10 300 python -u bench.py --steps 5 --warmup 1 --no-cpu-baseline \
    > $OUT/stamps.json 2> $OUT/stamps.err
rc=$?; echo "STAMPS rc=$rc"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('SMOKE OK')" > $OUT/smoke.log 2>&1
rc=$?; echo "SMOKE rc=$rc"; tail -2 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -u bench.py --full --profile c5 --nodes 100000 > $OUT/c5.json 2> $OUT/c5.err
rc=$?; echo "C5 rc=$rc"; cat $OUT/c5.json; [ $rc -eq 0 ] || { tail -3 $OUT/c5.err; exit $rc; }
