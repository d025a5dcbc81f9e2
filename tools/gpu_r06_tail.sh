#!/bin/bash
# Round 6: tail GEMMs on the deep register pipeline (gemm_deep.h, AAA_TAIL_DEEP=1) vs the one-stage
# gemm_kernel (=0), same build, same box: C2 and C3 lines, then the full -m gpu suite.
R=${GRAFT_REPO_ROOT:-$(pwd)}; O=$R/gpurun_out/r06tail; mkdir -p $O; cd $R; export TMPDIR=/tmp
run() {  # name config env...
  local n=$1 c=$2; shift 2
  env "$@" timeout -k 10 300 python bench.py --full --config $c --no-cpu-baseline --no-dropin --no-episode > $O/$n.json 2> $O/$n.err || { echo "bench $n rc=$?"; tail -3 $O/$n.err; exit 1; }
  python -c "
import json;d=json.loads(open('$O/$n.json').read().strip().splitlines()[-1]);k=d['kernels']
print('$n',d['value'],d['ms_per_step'],{n[:18]:round(v.get('ms',v.get('avg_us',0)/1e3),4) for n,v in k.items() if 'tail' in n or 'attn' in n})"
}
for c in c2 c3; do
  run ${c}_d0 $c AAA_TAIL_DEEP=0
  run ${c}_d1 $c AAA_TAIL_DEEP=1
  run ${c}_d0b $c AAA_TAIL_DEEP=0
  run ${c}_d1b $c AAA_TAIL_DEEP=1
done
timeout -k 10 900 python -u -m pytest -x -q --timeout 200 --timeout-method thread -m gpu tests > $O/tests.log 2>&1; rc=$?
tail -3 $O/tests.log; [ $rc -eq 0 ] || exit $rc
echo done
