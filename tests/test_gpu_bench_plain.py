"""bench.py's plain run and --dump-outputs.

A plain ``bench.py --gpus 1 --steps K --warmup W`` prints the headline line only
(no kernel table, no legs behind --full), and ``--dump-outputs DIR`` writes what
the last timed step computed.  The inputs are seeded, so the dumped arrays must
equal what the same Learner.step gives in this process on the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT, detinit, rel_err

pytestmark = pytest.mark.gpu

B, T, A = 4, 20, 18   # c2 at 4 rows: one process start and three 84x84 steps


def test_plain_line_and_dumped_outputs(cuda, tmp_path):
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--batch", str(B), "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stdout[-2000:] + p.stderr[-4000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - B * T / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"] + 1.0, d
    # what --full adds stays out of a plain line
    for key in ("roofline", "kernels", "hbm_kernels", "optimizer", "dropin", "episode", "cpu_baseline"):
        assert key not in d, key

    from aaa_amd.learner import Learner
    learner = Learner(B, T, 84, 84, 4, A, "fp32", cuda, frames_u8=True)
    frames = torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3))).to(cuda)
    dl = torch.from_numpy(detinit.normal(2, (T, B, A))).to(cuda)
    dv = torch.from_numpy(detinit.normal(3, (T, B, A))).to(cuda)
    lg, vl = learner.step(frames, dl, dv)
    torch.cuda.synchronize()
    want = {"logits": lg, "values": vl, "grads": learner.grads}
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in want)
    for name, t in want.items():
        a = np.load(out_dir / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(t.shape), (name, a.dtype, a.shape)
        assert np.all(np.isfinite(a)), name
        # same kernels on the same inputs; only the order of the gradients' atomic sums may differ
        assert rel_err(a, t.detach().cpu().numpy()) <= 1e-5, name
