# Full GPU pass: parity tests, smoke, bench (default and the driver's short form),
# rocprofv3 kernel trace + FETCH_SIZE / WRITE_SIZE passes.
set -u
TAG=${1:-r02}
export TMPDIR=/tmp
OUT=${OUT:-bench_out}   # where the records go
mkdir -p $OUT
timeout -k 10 1200 python -u -m pytest tests -q -m gpu -p no:cacheprovider --timeout 300 --timeout-method thread \
    > $OUT/gpu_tests_$TAG.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -3 $OUT/gpu_tests_$TAG.log
[ $rc -le 1 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 || exit $?
timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit $?
tail -1 $OUT/bench_$TAG.json
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_short_$TAG.json 2> $OUT/bench_short_$TAG.err || exit $?
ARGS="--full --steps 200 --warmup 20 --cpu-baseline 0 --alt-steps 50"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 bench.py $ARGS > $OUT/prof_$TAG.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc_fetch_$TAG -o run --output-format csv -- python3 bench.py --steps 10 --warmup 2 --cpu-baseline 0 --alt-steps 0 > $OUT/pmc_fetch_$TAG.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc_write_$TAG -o run --output-format csv -- python3 bench.py --steps 10 --warmup 2 --cpu-baseline 0 --alt-steps 0 > $OUT/pmc_write_$TAG.log 2>&1 || exit $?
grep -E "step_env|step_flat|flat_prime|advance_|scalar_step" $OUT/prof_$TAG/run_kernel_stats.csv | cut -c1-170
