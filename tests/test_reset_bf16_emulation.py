"""What the bf16-emulated oracle says about episode starts (tests/reset_ref.py over
oracle/ref_cpu.py, conv_mode="bf16"), pinned on the CPU so that the meaning of the
GPU gate in tests/test_gpu_resets_bf16.py is on record:

* a reset is a fresh start: with reset[s][:] = 1 the oracle equals two plain bf16
  unrolls of the segments, exactly;
* at T=5, B=4, 84x84 and the mask MASK54 of test_gpu_resets.py the mask moves the
  outputs by less than the 2e-2 bf16 gate (measured: logits 0.8 %, values 1.0 %,
  maps 0.75 % norm-relative), so an output comparison against the oracle cannot
  show that a mask was applied;
* it moves the gradients far beyond it (measured: 27 of the 32 non-zero tensors
  by >= 0.12, median 0.29), so the oracle test compares gradients, and the
  forward's selectivity is shown HIP-vs-HIP.
"""
import functools

import numpy as np
import torch

from helpers import detinit, rel_err
from oracle import ref_cpu

import reset_ref

MASK54 = ((0, 2), (2, 1), (4, 2), (1, 3), (2, 3))


def _frames(T, B):
    return torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3)).astype(np.float32))


def _mask(T, B, at):
    m = torch.zeros(T, B)
    for t, b in at:
        m[t, b] = 1.0
    return m


@functools.lru_cache(maxsize=None)
def _run(T, B, at):
    P = ref_cpu.tensor_params(detinit.deterministic_params(0, 18, 4))
    lg, vl, am, _ = reset_ref.unroll(P, _frames(T, B), _mask(T, B, at), conv_mode="bf16", kinks=ref_cpu.KinkProbe(None))
    Gl = torch.from_numpy(detinit.cotangent(2, (T, B, 18)))
    Gv = torch.from_numpy(detinit.cotangent(3, (T, B, 18)))
    ((lg * Gl).sum() + (vl * Gv).sum()).backward()
    return lg.detach(), vl.detach(), am.detach(), reset_ref.grads(P)


def test_a_full_reset_row_is_two_plain_unrolls():
    T, B, s = 4, 3, 2
    X = _frames(T, B)
    P = ref_cpu.tensor_params(detinit.deterministic_params(0, 18, 4), requires_grad=False)
    with torch.no_grad():
        one = reset_ref.unroll(P, X, _mask(T, B, [(s, b) for b in range(B)]), conv_mode="bf16")[:3]
        two = [ref_cpu.unroll(P, X[lo:hi], conv_mode="bf16") for lo, hi in ((0, s), (s, T))]
    for i, n in enumerate(("logits", "values", "attn")):
        assert torch.equal(one[i], torch.cat([two[0][i], two[1][i]])), n


def test_the_mask_moves_gradients_not_outputs():
    T, B = 5, 4
    masked, plain = _run(T, B, MASK54), _run(T, B, ())
    for i, n in enumerate(("logits", "values", "attn")):
        e = rel_err(masked[i].numpy(), plain[i].numpy())
        assert 0.0 < e < 2e-2, (n, e)
    moved = {n: rel_err(masked[3][n].numpy(), g.numpy()) for n, g in plain[3].items() if float(g.norm()) > 0}
    assert sum(e > 4e-2 for e in moved.values()) >= 20, sorted(moved.items(), key=lambda kv: kv[1])
