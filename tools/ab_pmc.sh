#!/bin/bash
R=${GRAFT_REPO_ROOT:-$(pwd)}; O=$R/gpurun_out; mkdir -p $O; cd $R
timeout -k 10 600 python -m pytest tests -m gpu -q -x -p no:cacheprovider > $O/parity.log 2>&1; rc=$?; echo "tests rc=$rc"; tail -3 $O/parity.log; [ $rc -le 1 ] || exit $rc
for v in 0 1; do
  AAA_STEP_TILE=$v timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 20 > $O/ab_$v.json 2>/dev/null; rc=$?; [ $rc -eq 0 ] || { echo "bench $v rc=$rc"; exit $rc; }
  python -c "import json;d=json.load(open('$O/ab_$v.json'));print('tile',$v,d['value'],d['ms_per_step'],json.dumps(d['kernels']))"
done
bash tools/pmc.sh
