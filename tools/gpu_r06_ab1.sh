#!/bin/bash
# Round 6 A/B 1: slot-matched zero pixels (fp32 pre-split recurrences) + row-padded bf16 forward h image.
R=${GRAFT_REPO_ROOT:-$(pwd)}; O=$R/gpurun_out/r06ab1; mkdir -p $O; cd $R
# the round-5 zero pixel on the P < 88 grid (expected to fail on the base library; recorded, not fatal)
AAA_LIB=$R/tools/ablibs/libaaa_base.so timeout -k 10 200 python -u -m pytest -x -q --timeout 120 --timeout-method thread -m gpu \
  "tests/test_gpu_f32_frames.py::test_f32_frames_small_grid_vs_oracle" > $O/base_small_grid.log 2>&1; echo "base small-grid rc=$?"
timeout -k 10 900 python -u -m pytest -x -v --timeout 300 --timeout-method thread -m gpu \
  tests/test_gpu_f32_frames.py tests/test_gpu_pairs.py tests/test_gpu_band.py \
  tests/test_gpu_bench_dp.py tests/test_gpu_share.py tests/test_gpu_coresidency.py \
  "tests/test_gpu_episode.py::test_long_actor_chain_episode_matches_oracle" \
  tests/test_gpu_parity.py > $O/tests.log 2>&1 || { echo "tests rc=$?"; tail -30 $O/tests.log; exit 1; }
tail -2 $O/tests.log; cp gpurun_out/kink_report.jsonl $O/ 2>/dev/null
for c in c2 c3 c4; do
  for arm in base new; do
    lib=$R/tools/ablibs/libaaa_base.so; [ $arm = new ] && lib=$R/towards-interpretable-reinforcement-learning-using-attention-augmented-agents-replication_amd/libaaa.so
    AAA_LIB=$lib timeout -k 10 300 python bench.py --full --config $c --no-cpu-baseline --no-dropin --no-episode > $O/${c}_$arm.json 2> $O/${c}_$arm.err || { echo "bench $c $arm rc=$?"; tail $O/${c}_$arm.err; exit 1; }
    python -c "import json;d=json.loads(open('$O/${c}_$arm.json').read().strip().splitlines()[-1]);print('$c $arm',d['value'],d['ms_per_step'],[(n[:22],v.get('avg_us',v.get('ms'))) for n,v in d['kernels'].items()][:3])"
  done
done
echo done
