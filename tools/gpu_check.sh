#!/bin/bash
# quick GPU session: full parity suite, then the default bench line
OUT=${UCF_TOOLS_OUT:-tools_out}     # logs, under the repository root
mkdir -p $OUT
timeout -k 10 ${PYTEST_TO:-1000} python -m pytest tests -m gpu -q --no-header -p no:cacheprovider ${PYTEST_ARGS:-} > $OUT/pytest_gpu.log 2>&1; rc=$?
echo "[pytest] rc=$rc"; grep -E "^(FAILED|ERROR)|passed|failed|Error" $OUT/pytest_gpu.log | tail -12; [ $rc -ne 0 ] && tail -60 $OUT/pytest_gpu.log
[ $rc -ge 124 ] && exit $rc
timeout -k 10 600 python bench.py --full > $OUT/bench_default.log 2> $OUT/bench_default.err; rc2=$?; echo "[bench] rc=$rc2"; tail -c 3000 $OUT/bench_default.log; tail -5 $OUT/bench_default.err
exit $rc
