#!/bin/bash
# The ensemble reduction kernels of the library built from the parent commit (PREV, default tools/ubench/libucf_prev.so, loaded
# through UCF_LIB_PATH) against the product, alternating on one box: per shape and run one process of
# tools/bench_ensemble_reduce.py --once under `rocprofv3 --kernel-trace --stats` (no counters), then --collect writes the report.
#   [ORDER="new parent"] tools/ensemble_reduce_ab.sh PARENT_COMMIT [OUT.json]     (ORDER: which build goes first in each pair)
PARENT=${1:?parent commit}; REPORT=${2:-profiles/ensemble_reduce_refactor.json}
PREV=${PREV:-$PWD/tools/ubench/libucf_prev.so}
OUT=$PWD/${UCF_TOOLS_OUT:-tools_out}/ensemble_reduce_ab; mkdir -p $OUT     # traces and logs, under the repository root
[ -f "$PREV" ] || { echo "no parent library at $PREV"; exit 2; }
UCF_LIB_PATH=$PREV timeout -k 10 120 python -c "from unconfined_amd import engine; print(engine.build_id())" > $OUT/parent.build_id || exit $?
timeout -k 10 120 python -c "from unconfined_amd import engine; print(engine.build_id())" > $OUT/new.build_id || exit $?
one() { # which, nens, nout, run
  local tag=$1_$2x$3_$4 envs=(X=1); [ $1 = parent ] && envs=(UCF_LIB_PATH=$PREV)
  env "${envs[@]}" timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$tag -- python tools/bench_ensemble_reduce.py --once $2 $3 > $OUT/$tag.log 2>&1; local rc=$?
  echo "[$tag] rc=$rc $(grep '^nens=' $OUT/$tag.log | tail -1)"
  [ $rc -ne 0 ] && { tail -5 $OUT/$tag.log; exit $rc; }
}
for shape in "64 262144" "512 65536" "1024 32768"; do
  for run in 1 2 3; do
    for which in ${ORDER:-parent new}; do one $which $shape $run; done
  done
done
timeout -k 10 120 python tools/bench_ensemble_reduce.py --collect $OUT $REPORT $PARENT
