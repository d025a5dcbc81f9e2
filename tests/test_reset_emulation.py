"""Pins the reference of the episode-start masks (tests/reset_ref.py) on the
CPU: with no resets it is ``oracle.ref_cpu.unroll`` over T; with a whole row
of resets at step s it is two independent unrolls of s and T-s steps (outputs
and summed gradients); a NaN state under a reset reaches nothing; and
``vtrace.episode_starts`` is its definition.  T=4, B=2 at 84x84; both sides
are the same fp32 torch code, asserted at the project's fp32 gate RTOL = 1e-4
(tests/test_gpu_parity.py).  Largest relative difference seen: 0, outputs and
summed gradients alike (the same op sequence on both sides).
"""
import numpy as np
import pytest
import torch

from helpers import assert_close, detinit, rel_err
from oracle import ref_cpu

import attention  # noqa: F401  (registers aaa_amd)
import reset_ref

RTOL = 1e-4   # tests/test_gpu_parity.py:18
T, B, S = 4, 2, 2


def _params():
    return ref_cpu.tensor_params(detinit.deterministic_params(0, 18, 4))


def _frames():
    return torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3)).astype(np.float32))


def _cot():
    return torch.from_numpy(detinit.cotangent(2, (T, B, 18))), torch.from_numpy(detinit.cotangent(3, (T, B, 18)))


def _loss(lg, vl, Gl, Gv):
    return (lg * Gl).sum() + (vl * Gv).sum()


@pytest.fixture(scope="module", params=[False, True], ids=["zero-core", "stateful-core"])
def plain(request):
    """ref_cpu.unroll over T from reset(): outputs and gradients, computed once."""
    sc = request.param
    P = _params()
    Gl, Gv = _cot()
    lg, vl, at = ref_cpu.unroll(P, _frames(), stateful_core=sc)
    _loss(lg, vl, Gl, Gv).backward()
    return sc, lg.detach(), vl.detach(), at.detach(), {n: g.clone() for n, g in reset_ref.grads(P).items()}


def _close(a, b, what):
    worst = 0.0
    for x, y, n in zip(a[:3], b[:3], ("logits", "values", "attn")):
        assert_close(x.numpy(), y.numpy(), RTOL, f"{what} {n}")
        worst = max(worst, rel_err(x.numpy(), y.numpy()))
    for n in b[3]:
        if float(b[3][n].norm()) == 0.0:
            assert float(a[3][n].abs().max()) == 0.0, n
        else:
            assert_close(a[3][n].numpy(), b[3][n].numpy(), RTOL, f"{what} grad {n}")
            worst = max(worst, rel_err(a[3][n].numpy(), b[3][n].numpy()))
    print(f"{what}: largest relative difference {worst:.2e}")


def test_no_resets_is_the_plain_unroll(plain):
    sc, *ref = plain
    P = _params()
    Gl, Gv = _cot()
    lg, vl, at, _ = reset_ref.unroll(P, _frames(), torch.zeros(T, B), stateful_core=sc)
    _loss(lg, vl, Gl, Gv).backward()
    _close((lg.detach(), vl.detach(), at.detach(), reset_ref.grads(P)), ref, "no resets")


@pytest.mark.parametrize("sc", [False, True], ids=["zero-core", "stateful-core"])
def test_row_of_resets_is_two_unrolls(sc):
    X = _frames()
    Gl, Gv = _cot()
    reset = torch.zeros(T, B)
    reset[S] = 1.0
    P = _params()
    lg, vl, at, _ = reset_ref.unroll(P, X, reset, stateful_core=sc)
    _loss(lg, vl, Gl, Gv).backward()
    Q = _params()
    a = ref_cpu.unroll(Q, X[:S], stateful_core=sc)
    b = ref_cpu.unroll(Q, X[S:], stateful_core=sc)
    (_loss(a[0], a[1], Gl[:S], Gv[:S]) + _loss(b[0], b[1], Gl[S:], Gv[S:])).backward()
    two = tuple(torch.cat([x, y]).detach() for x, y in zip(a, b)) + (reset_ref.grads(Q),)
    _close((lg.detach(), vl.detach(), at.detach(), reset_ref.grads(P)), two, "two segments")


@pytest.mark.parametrize("sc", [False, True], ids=["zero-core", "stateful-core"])
def test_nan_state_under_a_reset_reaches_nothing(sc):
    X = _frames()
    h, w = ref_cpu.grid_of(84, 84)
    nan = float("nan")
    state = tuple(torch.full((B, 128, w, h), nan if i == 0 else 0.0) for i in range(2))
    state = tuple(s.index_fill(0, torch.tensor([1]), 0.0).requires_grad_() for s in state)   # row 0 NaN, row 1 zeros
    core = tuple(torch.full((B, 256), nan).index_fill(0, torch.tensor([1]), 0.0).requires_grad_()
                 for _ in range(2)) if sc else None
    reset = torch.zeros(T, B)
    reset[0, 0] = 1.0
    P = _params()
    Gl, Gv = _cot()
    lg, vl, at, _ = reset_ref.unroll(P, X, reset, state=state, core_state=core, stateful_core=sc)
    assert all(bool(torch.isfinite(x).all()) for x in (lg, vl, at))
    _loss(lg, vl, Gl, Gv).backward()
    assert all(bool(torch.isfinite(g).all()) for g in reset_ref.grads(P).values())
    for s in state + (core or ()):
        assert float(s.grad[0].abs().max()) == 0.0   # the reset row's state cotangent is exactly 0
    assert float(state[0].grad[1].abs().max()) > 0.0


def test_episode_starts_matches_its_definition():
    from aaa_amd import vtrace as vt
    done = torch.from_numpy((detinit.frames_u8(5, (T, B)) % 2).astype(np.float32))
    for first in (None, torch.tensor([1.0, 0.0])):
        got = vt.episode_starts(done, first)
        want = torch.zeros(T, B)
        if first is not None:
            want[0] = first
        for t in range(1, T):
            want[t] = done[t - 1]
        assert got.dtype == torch.float32 and tuple(got.shape) == (T, B) and torch.equal(got, want)
