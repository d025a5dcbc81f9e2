"""Episode starts inside an fp32 unroll (include/aaa.h aaa_forward_resets /
aaa_backward_resets; csrc/resets.hip): ``reset[t][b] != 0`` puts row b into
the reset() state before step t -- what the reference does with
``agent.reset()`` at an episode start (main_mp.py:100), per row.  Against
tests/reset_ref.py (oracle.ref_cpu.unroll composed step by step) at the fp32
gate RTOL = 1e-4, against plain unrolls of the segments at the HIP-vs-HIP
figure 1e-5, and bit for bit where the same kernels run.

With a mask the forward runs the frame-group kernels' mask variants (G = 8
pre-split, G = 4) or the per-step kernels, and the BPTT the frame-group
kernel's mask variant (G = 8) or the per-step chain; the variant strings name
the kernel with ", resets".  The default dispatch takes the frame-group kernels
only from about half a chip of workgroups on (rt_core.hip f32_frames), so the
small batches here reach them through AAA_F32_FRAMES=8 / 4.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_close, detinit, rel_err
from oracle import ref_cpu
from test_gpu_parity import RTOL, _agent, _compare, _cot, _frames, _grads

import attention
import reset_ref
from aaa_amd.runtime import UnrollRunner
from aaa_amd.vtrace import episode_starts

pytestmark = pytest.mark.gpu
N = attention._pkg._native

# B=4, T=5: row 0 never, row 1 at t=2, row 2 at t=0 and at the last step, row 3 at two consecutive steps
MASK54 = ((0, 2), (2, 1), (4, 2), (1, 3), (2, 3))


def _mask(T, B, at):
    m = torch.zeros(T, B)
    for t, b in at:
        m[t, b] = 1.0
    return m


@functools.lru_cache(maxsize=None)
def _ref(T, B, at, H=84, W=84):
    """reset_ref's outputs and gradients for a mask, computed once per case."""
    P = ref_cpu.tensor_params(detinit.deterministic_params(0, 18, 4))
    lg, vl, a, _ = reset_ref.unroll(P, _frames(T, B, H, W), _mask(T, B, at))
    Gl, Gv = _cot(T, B)
    ((lg * Gl).sum() + (vl * Gv).sum()).backward()
    return lg.detach(), vl.detach(), a.detach(), reset_ref.grads(P)


def _run(agent, X, reset, dev, fresh=True):
    """One unroll + backward on the HIP path: (logits, values, attn, grads) on the host."""
    T, B = X.shape[:2]
    if fresh:
        agent.reset()
    agent.zero_grad()
    lg, vl, at = agent.unroll(X.to(dev), reset=None if reset is None else reset.to(dev))
    Gl, Gv = _cot(T, B)
    ((lg * Gl.to(dev)).sum() + (vl * Gv.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return lg.detach().cpu(), vl.detach().cpu(), at.detach().cpu(), _grads(agent)


def _timed(fn):
    N.timing_enable(True)
    try:
        out = fn()
        return out, N.timing_stats(N.TIMER_FWD_STEP)["variant"], N.timing_stats(N.TIMER_BPTT_STEP)["variant"]
    finally:
        N.timing_enable(False)


CASES = {
    # name: (env, T, B, mask, H, W, grid)
    "G8": ({"AAA_F32_FRAMES": "8"}, 5, 4, MASK54, 84, 84, (11, 11)),
    "G4": ({"AAA_F32_FRAMES": "4"}, 5, 4, MASK54, 84, 84, (11, 11)),
    "per-step": ({"AAA_F32_FRAMES": "0"}, 5, 4, MASK54, 84, 84, (11, 11)),
    "per-step fused-x": ({"AAA_F32_FRAMES": "0", "AAA_FUSED_X": "1"}, 5, 4, MASK54, 84, 84, (11, 11)),
    "per-step batched-x": ({"AAA_F32_FRAMES": "0", "AAA_FUSED_X": "0"}, 5, 4, MASK54, 84, 84, (11, 11)),
    "G8 ragged column": ({"AAA_F32_FRAMES": "8"}, 3, 9, ((1, 8), (2, 3)), 84, 84, (11, 11)),
    "G8 8x8 grid": ({"AAA_F32_FRAMES": "8"}, 4, 3, ((1, 0), (3, 2), (0, 1)), 64, 64, (8, 8)),
    "210x160": ({}, 3, 1, ((1, 0),), 210, 160, (27, 20)),
}
# the forward kernel each case must name
FWD_KERNEL = {"G8": "8 WG per frame [kernel: k_convlstm_fwd_f32ps]", "G4": "4 WG per frame [kernel: k_convlstm_fwd_f32<]",
              "G8 ragged column": "8 WG per frame [kernel: k_convlstm_fwd_f32ps]",
              "G8 8x8 grid": "8 WG per frame [kernel: k_convlstm_fwd_f32ps]"}
# ... and the BPTT kernel: the frame-group BPTT at G = 8, else the per-step chain
BWD_KERNEL = {c: "8 WG per frame [kernel: k_convlstm_bwd_f32]" for c in ("G8", "G8 ragged column", "G8 8x8 grid")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_core_paths_vs_reference(cuda, monkeypatch, case):
    env, T, B, at, H, W, grid = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    agent = _agent(cuda, grid=grid)
    out, var, bvar = _timed(lambda: _run(agent, _frames(T, B, H, W), _mask(T, B, at), cuda))
    assert FWD_KERNEL.get(case, "EpiConvLstmFwd") in var and var.endswith(", resets"), var
    assert BWD_KERNEL.get(case, "EpiConvLstmBwd") in bvar and bvar.endswith(", resets"), bvar
    if "FUSED_X" in env:
        assert ("fused [x|h] step" in var) == (env["AAA_FUSED_X"] == "1"), var
    _compare(out, _ref(T, B, at, H, W), RTOL, f"resets {case}: ")
    assert N.pair_status(clear=True) == 0


def test_no_mask_variants_unchanged(cuda, monkeypatch):
    """reset=None launches what it launched before: the frame-group kernels, their strings as they were."""
    monkeypatch.setenv("AAA_F32_FRAMES", "8")
    _, var, bvar = _timed(lambda: _run(_agent(cuda), _frames(3, 4), None, cuda))
    assert "8 WG per frame" in var and "frame-group BPTT" in bvar and "resets" not in var + bvar, (var, bvar)
    assert N.pair_status(clear=True) == 0


@pytest.mark.parametrize("G", ["8", "0"])
def test_segment_equivalence(cuda, monkeypatch, G):
    """reset[s][:] = 1: one unroll of T steps against two plain unrolls of s and T-s steps from reset()."""
    monkeypatch.setenv("AAA_F32_FRAMES", G)
    T, B, s = 5, 3, 2
    X = _frames(T, B)
    Gl, Gv = _cot(T, B)
    agent = _agent(cuda)
    one = _run(agent, X, _mask(T, B, [(s, b) for b in range(B)]), cuda)
    agent.zero_grad()
    parts = []
    for lo, hi in ((0, s), (s, T)):
        agent.reset()
        lg, vl, at = agent.unroll(X[lo:hi].to(cuda))
        ((lg * Gl[lo:hi].to(cuda)).sum() + (vl * Gv[lo:hi].to(cuda)).sum()).backward()
        parts.append((lg.detach().cpu(), vl.detach().cpu(), at.detach().cpu()))
    torch.cuda.synchronize()
    two = _grads(agent)
    for i, n in enumerate(("logits", "values", "attn")):
        assert_close(one[i].numpy(), torch.cat([parts[0][i], parts[1][i]]).numpy(), 1e-5, f"G={G} segments {n}")
    for n in two:
        if float(two[n].norm()) > 0:
            assert rel_err(one[3][n].numpy(), two[n].numpy()) <= 1e-5, f"G={G} segments grad {n}"
    assert N.pair_status(clear=True) == 0
    if G != "0":
        return
    # the second segment continued from the first's state with reset[0][:] = 1: autograd hands its
    # dh0 / dc0 (exactly 0) to the first segment as dhT / dcT -- the gradients must not move
    agent.zero_grad()
    agent.reset()
    a = agent.unroll(X[:s].to(cuda))
    b = agent.unroll(X[s:].to(cuda), reset=_mask(T - s, B, [(0, b) for b in range(B)]).to(cuda))
    ((a[0] * Gl[:s].to(cuda)).sum() + (a[1] * Gv[:s].to(cuda)).sum() + (b[0] * Gl[s:].to(cuda)).sum()
     + (b[1] * Gv[s:].to(cuda)).sum()).backward()
    torch.cuda.synchronize()
    chained = _grads(agent)
    for n in two:
        if float(two[n].norm()) > 0:
            assert rel_err(chained[n].numpy(), one[3][n].numpy()) <= 1e-5, f"chained segments grad {n}"


@pytest.mark.parametrize("G", ["0", "8"])
def test_all_zero_mask_is_no_mask(cuda, monkeypatch, G):
    """The forward is bit-identical (G = 0: the same step kernels; G = 8: the frame-group kernel and its
    mask variant, the same operations in the same order); the gradients agree at 1e-5."""
    monkeypatch.setenv("AAA_F32_FRAMES", G)
    T, B = 4, 3
    agent = _agent(cuda)
    none = _run(agent, _frames(T, B), None, cuda)
    zero = _run(agent, _frames(T, B), torch.zeros(T, B), cuda)
    for i, n in enumerate(("logits", "values", "attn")):
        assert torch.equal(none[i], zero[i]), f"G={G}: zero mask moved {n}"
    for n in none[3]:
        if float(none[3][n].norm()) > 0:
            assert rel_err(zero[3][n].numpy(), none[3][n].numpy()) <= 1e-5, f"zero mask grad {n}"
    assert N.pair_status(clear=True) == 0


@pytest.mark.parametrize("G", ["8", "4", "0"])
def test_frames_before_a_reset_reach_nothing_after_it(cuda, monkeypatch, G):
    monkeypatch.setenv("AAA_F32_FRAMES", G)
    T, B = 5, 4
    mask = _mask(T, B, MASK54)
    agent = _agent(cuda)
    X = _frames(T, B)
    a = _run(agent, X, mask, cuda)
    Y = X.clone()
    Y[:2, 1] = torch.from_numpy(detinit.frames_u8(99, (2, 84, 84, 3)).astype(np.float32))   # row 1 resets at t = 2
    b = _run(agent, Y, mask, cuda)
    for i, n in enumerate(("logits", "values", "attn")):
        assert torch.equal(a[i][2:, 1], b[i][2:, 1]), f"row 1 {n} after its reset"
        assert not torch.equal(a[i][:2, 1], b[i][:2, 1])


def _state(B, nan_row, dev, seed):
    """A carried ConvLSTM state in the agent's (B, 128, w, h) layout, one row NaN."""
    s = torch.from_numpy(detinit.cotangent(seed, (B, 128, 11, 11))).clone()
    s[nan_row] = float("nan")
    return s.to(dev).requires_grad_()


@pytest.mark.parametrize("G", ["8", "4", "0"])
def test_nan_state_under_a_reset(cuda, monkeypatch, G):
    """G = 0: reset=None runs the same step kernels, so the other rows' state gradients are compared exactly;
    G = 8 / 4: the frame-group kernels and their mask variants (HIP vs HIP, 1e-5)."""
    monkeypatch.setenv("AAA_F32_FRAMES", G)
    T, B, row = 3, 3, 1
    X = _frames(T, B).to(cuda)
    Gl, Gv = (c.to(cuda) for c in _cot(T, B))
    agent = _agent(cuda)
    cell = agent.vision.vision_lstm

    def run(h, c, reset):
        agent.reset()
        agent.zero_grad()
        cell.prev_hidden = (h, c)
        lg, vl, at = agent.unroll(X, reset=reset)
        ((lg * Gl).sum() + (vl * Gv).sum()).backward()
        torch.cuda.synchronize()
        return lg.detach().cpu(), vl.detach().cpu(), at.detach().cpu(), h.grad.cpu(), c.grad.cpu()

    mask = _mask(T, B, [(0, row), (2, 0)]).to(cuda)
    nan = run(_state(B, row, cuda, 41), _state(B, row, cuda, 42), mask)
    # the zero-state run: zeros in that row, no reset at its step 0
    hz, cz = (torch.nan_to_num(_state(B, row, cuda, k).detach(), nan=0.0).requires_grad_() for k in (41, 42))
    zero = run(hz, cz, _mask(T, B, [(2, 0)]).to(cuda))
    for i, n in enumerate(("logits", "values", "attn")):
        assert bool(torch.isfinite(nan[i]).all()) and torch.equal(nan[i], zero[i]), n
    for g in nan[3:]:
        assert float(g[row].abs().max()) == 0.0
    # the other rows' dh0 / dc0: the no-mask run's (rows 0 and 2; row 0 resets at t = 2 in ``mask``, so
    # compare under the mask that only cuts row ``row`` at step 0)
    only = run(_state(B, row, cuda, 41), _state(B, row, cuda, 42), _mask(T, B, [(0, row)]).to(cuda))
    hz, cz = (torch.nan_to_num(_state(B, row, cuda, k).detach(), nan=0.0).requires_grad_() for k in (41, 42))
    none = run(hz, cz, None)
    for i in (3, 4):
        for b in (0, 2):
            if G == "0":
                assert torch.equal(only[i][b], none[i][b]), (i, b)
            else:
                assert_close(only[i][b].numpy(), none[i][b].numpy(), 1e-5, f"G={G} state grad {i} row {b}")
        assert float(only[i][row].abs().max()) == 0.0
        assert float(none[i][row].abs().max()) > 0.0


@pytest.mark.parametrize("G", ["8", "0"])
def test_stateful_core_vs_reference(cuda, monkeypatch, G):
    """Core state carried in and out; core_h0 holds NaN in a row with reset[0]."""
    monkeypatch.setenv("AAA_F32_FRAMES", G)
    T, B = 5, 3
    at = ((0, 1), (2, 0), (3, 0), (4, 2))
    mask = _mask(T, B, at)
    ch = torch.from_numpy(detinit.cotangent(51, (B, 256))).clone()
    cc = torch.from_numpy(detinit.cotangent(52, (B, 256))).clone()
    P = ref_cpu.tensor_params(detinit.deterministic_params(0, 18, 4))
    Gl, Gv = _cot(T, B)
    rch, rcc = ch.clone().requires_grad_(), cc.clone().requires_grad_()
    rl, rv, ra, (_, rcore) = reset_ref.unroll(P, _frames(T, B), mask, core_state=(rch, rcc), stateful_core=True)
    Gc = torch.from_numpy(detinit.cotangent(53, (B, 256)))
    ((rl * Gl).sum() + (rv * Gv).sum() + (rcore[0] * Gc).sum() + (rcore[1] * Gc).sum()).backward()
    ref = (rl.detach(), rv.detach(), ra.detach(), reset_ref.grads(P))

    agent = attention.Agent(18, grid=(11, 11), stateful_core=True)
    detinit.load_into(agent, detinit.deterministic_params(0, 18, 4))
    agent.to(cuda)
    agent.reset()
    h0 = ch.clone()
    h0[1] = float("nan")   # row 1 starts an episode at step 0: never read
    h0, c0 = h0.to(cuda).requires_grad_(), cc.to(cuda).requires_grad_()
    agent.prev_output, agent.prev_hidden = h0, c0
    lg, vl, am = agent.unroll(_frames(T, B).to(cuda), reset=mask.to(cuda))
    g = Gc.to(cuda)
    ((lg * Gl.to(cuda)).sum() + (vl * Gv.to(cuda)).sum() + (agent.prev_output * g).sum()
     + (agent.prev_hidden * g).sum()).backward()
    torch.cuda.synchronize()
    _compare((lg.detach().cpu(), vl.detach().cpu(), am.detach().cpu(), _grads(agent)), ref, RTOL, "stateful resets: ")
    assert_close(agent.prev_output.detach().cpu().numpy(), rcore[0].detach().numpy(), RTOL, "core hT")
    assert_close(agent.prev_hidden.detach().cpu().numpy(), rcore[1].detach().numpy(), RTOL, "core cT")
    for got, want, n in ((h0.grad, rch.grad, "dcore_h0"), (c0.grad, rcc.grad, "dcore_c0")):
        assert float(got[1].abs().max()) == 0.0, n
        assert_close(got.cpu().numpy(), want.numpy(), RTOL, n)
    assert N.pair_status(clear=True) == 0


def test_agent_unroll_matches_the_runner(cuda, monkeypatch):
    monkeypatch.setenv("AAA_F32_FRAMES", "8")
    T, B = 5, 4
    mask = _mask(T, B, MASK54).to(cuda)
    agent = _agent(cuda)
    X = _frames(T, B).to(cuda)
    out = _run(agent, X, mask, cuda)
    r = UnrollRunner(B, T, 84, 84, device=cuda)
    flat = torch.cat([p.detach().reshape(-1) for p in agent.parameters()])
    packed, ws = r.new_packed(), r.new_workspace()
    r.pack(flat, packed)
    S = agent.spatial.S.to(cuda).contiguous()
    lg, vl, at, _, _ = r.forward(flat, packed, S, X, ws, reset=mask)
    Gl, Gv = _cot(T, B)
    grads, _, _ = r.backward(flat, packed, S, X, ws, Gl.to(cuda), Gv.to(cuda), reset=mask)
    torch.cuda.synchronize()
    assert torch.equal(lg.cpu(), out[0]) and torch.equal(vl.cpu(), out[1]) and torch.equal(at.cpu(), out[2])
    mine = torch.cat([out[3][n].reshape(-1) for n, _ in agent.named_parameters()])
    assert rel_err(grads.cpu().numpy(), mine.numpy()) <= 1e-5


def test_learner_reset_done(cuda, monkeypatch):
    from aaa_amd.learner import Learner
    monkeypatch.setenv("AAA_F32_FRAMES", "8")   # the frame-group kernels, as a production batch runs them
    T, B = 5, 3
    frames = _frames(T, B).to(cuda).contiguous()
    actions = torch.from_numpy((detinit.frames_u8(7, (T, B)) % 18).astype(np.int32)).to(cuda)
    rewards = torch.from_numpy(detinit.cotangent(8, (T, B))).to(cuda)
    blogp = -torch.from_numpy(detinit.cotangent(9, (T, B))).abs().to(cuda)
    done = _mask(T, B, [(1, 0), (3, 2)]).to(cuda)

    def step(done, **kw):
        lr = Learner(B=B, T=T, device=cuda)
        lg, _, _ = lr.train_step_vtrace(frames, actions, rewards, blogp, done, "last", **kw)
        torch.cuda.synchronize()
        lr.check_health()
        return lg.cpu(), lr.grads.cpu().clone()

    by_name = step(done, reset="done")
    explicit = step(done, reset=episode_starts(done))
    none = step(done)
    # the same launches on the same mask; the weight gradients are split-K atomic sums, whose order
    # moves between two runs of anything (test_gpu_parity.py test_repeat_is_deterministic_enough)
    assert torch.equal(by_name[0], explicit[0])
    assert rel_err(by_name[1].numpy(), explicit[1].numpy()) <= 1e-5
    # done at (1, 0) and (3, 2): steps 0-1 are reset=None's (the plain kernel against its mask variant,
    # 1e-5), row 0 from step 2 on is not
    assert_close(by_name[0][:2].numpy(), none[0][:2].numpy(), 1e-5, "before the first done")
    assert rel_err(by_name[0][2:, 0].numpy(), none[0][2:, 0].numpy()) > 1e-3
    assert rel_err(by_name[1].numpy(), none[1].numpy()) > 1e-3
    first = step(done, reset="done", first=torch.tensor([0.0, 1.0, 0.0], device=cuda))
    assert torch.equal(first[0], by_name[0])   # the learner's unroll starts from reset() anyway
    # no done inside the unroll: the forward is reset=None's bit for bit (the frame-group kernel and its mask
    # variant: the same operations in the same order); the gradients are atomic sums (1e-5)
    quiet = torch.zeros(T, B, device=cuda)
    a, b = step(quiet, reset="done"), step(quiet)
    assert torch.equal(a[0], b[0])
    assert rel_err(a[1].numpy(), b[1].numpy()) <= 1e-5
