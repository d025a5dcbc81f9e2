#!/bin/bash
# Round 5 end-of-round measurements: the default bench line (C2 + drop-in + episode + CPU baseline),
# the C3 / C4 / C5 lines, and a kernel trace of the default C2 line at the bench's own steps.
R=${GRAFT_REPO_ROOT:-$(pwd)}; O=$R/gpurun_out/r05final; mkdir -p $O; cd $R
timeout -k 10 400 python bench.py --full > $O/c2_bench.json 2> $O/c2_bench.err || { echo "c2 rc=$?"; exit 1; }
for c in c3 c4 c5; do
  timeout -k 10 300 python bench.py --full --config $c --no-cpu-baseline --no-episode > $O/${c}_bench.json 2> $O/${c}_bench.err || { echo "$c rc=$?"; exit 1; }
done
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/prof_c2 -o run --output-format csv -- python $R/bench.py --full --no-cpu-baseline --no-dropin --no-episode > $O/c2_prof.json 2> $O/c2_prof.err || { echo "prof rc=$?"; exit 1; }
python $R/tools/trace_vs_events.py $O/prof_c2/run_kernel_trace.csv $O/c2_prof.json 1 > $O/c2_cmp.json || exit 1
for c in c2 c3 c4 c5; do python -c "
import json;d=json.loads(open('$O/${c}_bench.json').read().strip().splitlines()[-1])
print('$c', d['value'], d['ms_per_step'], d['roofline']['kernel'], d['roofline']['frac'], d.get('job_roofline',{}).get('frac'), (d.get('episode') or {}).get('episode_frames_per_s'))"; done
echo done
