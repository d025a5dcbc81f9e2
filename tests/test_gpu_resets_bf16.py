"""Episode starts inside a bf16 unroll (AAA_FLAG_BF16_RESETS, include/aaa.h;
``Agent(conv_dtype="bf16", resets=True)``, ``UnrollRunner(resets=True)``,
``Learner(dtype="bf16", resets=True)``).

Under a mask the forward runs the single-workgroup frame-resident kernel's mask
variant (recur.h RST) where the forward's rule gives one workgroup per frame,
behind it the BPTT runs the single-workgroup frame-resident kernel's mask
variant (recur_bwd.h RST) where AAA_FRAMES_BWD's rule gives 1, and the per-step
kernels run everywhere else.  Paired and band-mode kernels are never launched
under a mask.  Every h_t is also stored in the HR region, which the readout
reads.

What discriminates (tests/test_reset_bf16_emulation.py pins it on the CPU): the
mask moves the bf16 oracle's outputs by less than the 2e-2 bf16 gate and its
gradients far beyond it, so the oracle test is a gradient test, and that the
forward applied the mask is shown HIP-vs-HIP (segments, frames replaced before
a reset, NaN state).

HIP-vs-HIP gradient bound: the weight gradients are atomic sums, so two
identical plain bf16 runs differ; each test measures that spread with the
unmasked kernels and allows max(1e-5, 4 x spread).  Measured spread on the
MI355X (largest norm-relative difference over the 32 non-zero tensors, two
identical plain runs): 1.9e-7 to 3.0e-7 over twelve measurements, so the bound
is 1e-5; the masked runs differed from their plain counterparts by at most
3.3e-7 (segments, frame-resident forward and BPTT), 2.7e-7 (segments, per-step)
and 2.3e-7 (all-zero mask), their outputs by exactly 0.
"""
import numpy as np
import pytest
import torch

from helpers import assert_close, detinit, oracle_masks, rel_err
from oracle import ref_cpu
from test_gpu_parity import _compare, _cot, _frames, _grads

import attention
import reset_ref
from aaa_amd.runtime import UnrollRunner
from aaa_amd.vtrace import episode_starts

pytestmark = pytest.mark.gpu
N = attention._pkg._native
BF16_RTOL = 2e-2   # the project's bf16 gate (test_gpu_parity._bf16_checked)

# B=4, T=5: row 0 never, row 1 at t=2, row 2 at t=0 and at the last step, row 3 at two consecutive steps
MASK54 = ((0, 2), (2, 1), (4, 2), (1, 3), (2, 3))
STEPS35 = ((1, 4), (2, 0), (0, 2))
FRAMES = {"AAA_FRAMES_FWD": "1", "AAA_FRAMES_BWD": "1"}
CASES = {
    # name: (env, T, B, mask, H, W, grid)
    "frames": (FRAMES, 5, 4, MASK54, 84, 84, (11, 11)),                       # P = 121: a ragged fourth column block
    "frames 8x8": (FRAMES, 4, 3, ((1, 0), (3, 2), (0, 1)), 64, 64, (8, 8)),   # two empty column blocks
    "frames fwd only": ({"AAA_FRAMES_FWD": "1", "AAA_FRAMES_BWD": "0"}, 5, 4, MASK54, 84, 84, (11, 11)),
    "steps": ({"AAA_FRAMES_FWD": "0"}, 3, 5, STEPS35, 84, 84, (11, 11)),      # M = 605: ragged tiles
    "steps batched-x": ({"AAA_FRAMES_FWD": "0", "AAA_FUSED_X": "0"}, 3, 5, STEPS35, 84, 84, (11, 11)),   # fp32 gates
    # the VALU readout kernels on the HR copy's dense rows of 128 (the MFMA forward is the default)
    "steps valu readout": ({"AAA_FRAMES_FWD": "0", "AAA_ATTN_MFMA": "0"}, 3, 5, STEPS35, 84, 84, (11, 11)),
    "pair->steps": ({"AAA_FRAMES_FWD": "2", "AAA_FRAMES_BWD": "2"}, 2, 9, ((1, 8),), 84, 84, (11, 11)),
    "band->steps": ({}, 3, 2, ((1, 0), (2, 1)), 168, 168, (21, 21)),
}
# the kernels a masked call of each case must name: the frame-resident ones, else the per-step chains
FWD_KERNEL = {c: "1 WG per frame [kernel: k_convlstm_fwd_frames" for c in ("frames", "frames 8x8", "frames fwd only")}
BWD_KERNEL = {c: "1 WG per frame, fp16 gates [kernel: k_convlstm_bwd_frames" for c in ("frames", "frames 8x8")}
# the HIP-vs-HIP comparisons: the frame-resident forward and BPTT / the per-step chains
HIP_ENV = {"frames": FRAMES, "steps": {"AAA_FRAMES_FWD": "0"}}


def _mask(T, B, at):
    m = torch.zeros(T, B)
    for t, b in at:
        m[t, b] = 1.0
    return m


def _agent(dev, grid=(11, 11), resets=True, stateful=False):
    ag = attention.Agent(18, grid=grid, conv_dtype="bf16", resets=resets, stateful_core=stateful)
    detinit.load_into(ag, detinit.deterministic_params(0, 18, 4))
    return ag.to(dev)


def _run(agent, X, reset, dev):
    """One unroll + backward from reset(): (logits, values, attn, grads) on the host."""
    T, B = X.shape[:2]
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


def _setenv(monkeypatch, env):
    for k in ("AAA_FRAMES_FWD", "AAA_FRAMES_BWD", "AAA_FUSED_X", "AAA_ATTN_MFMA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _oracle(T, B, mask, masks, H=84, W=84, **kw):
    """reset_ref through the bf16-emulated oracle and the HIP path's own ReLU masks (the mask-matched
    oracle, as test_gpu_parity._oracle): a 5-tuple for _compare."""
    P = ref_cpu.tensor_params(detinit.deterministic_params(0, 18, 4))
    probe = ref_cpu.KinkProbe(masks)
    lg, vl, am, final = reset_ref.unroll(P, _frames(T, B, H, W), mask, conv_mode="bf16", kinks=probe, **kw)
    diag = {"env": {}, "units": [], "mismatch": probe.mismatch, "mismatch_pre": probe.mismatch_pre,
            "compared": probe.units, "masked": True}
    return P, (lg, vl, am), final, diag


def _spread_bound(agent, X, dev):
    """max(1e-5, 4 x the spread of two identical plain runs): the HIP-vs-HIP gradient bound."""
    a, b = _run(agent, X, None, dev), _run(agent, X, None, dev)
    for i in range(3):
        assert torch.equal(a[i], b[i])
    spread = max(rel_err(a[3][n].numpy(), b[3][n].numpy()) for n in a[3] if float(b[3][n].norm()) > 0)
    print(f"plain bf16 repeat spread (max over tensors, norm-relative): {spread:.3e}")
    return max(1e-5, 4 * spread), a


def _grads_close(got, want, bound, what):
    errs = {n: rel_err(got[n].numpy(), want[n].numpy()) for n in want if float(want[n].norm()) > 0}
    worst = sorted(errs.items(), key=lambda kv: -kv[1])
    print(f"{what}: gradient differences, worst first: " + ", ".join(f"{n} {e:.2e}" for n, e in worst[:40]))
    for n in want:
        if float(want[n].norm()) == 0:
            assert float(got[n].abs().max()) == 0.0, f"{what}: grad {n}"
    assert worst[0][1] <= bound, f"{what}: grad {worst[0][0]} differs by {worst[0][1]:.3e} > {bound:.1e}"


@pytest.mark.parametrize("case", sorted(CASES))
def test_core_paths_vs_bf16_oracle(cuda, monkeypatch, case):
    """(a) the kernels a masked call names, (b) outputs and gradients against the mask-matched bf16 oracle."""
    env, T, B, at, H, W, grid = CASES[case]
    _setenv(monkeypatch, env)
    agent = _agent(cuda, grid=grid)
    agent.relu_trace = []
    mask = _mask(T, B, at)
    out, var, bvar = _timed(lambda: _run(agent, _frames(T, B, H, W), mask, cuda))
    assert FWD_KERNEL.get(case, "EpiConvLstmFwd") in var and var.endswith(", resets"), var
    assert BWD_KERNEL.get(case, "EpiConvLstmBwd") in bvar and bvar.endswith(", resets"), bvar
    assert "bands per frame" not in var + bvar and "2 WG per frame" not in var + bvar and "pairs" not in bvar, (var, bvar)
    if "AAA_FUSED_X" in env:
        assert "h-part step (x-part batched)" in var and "fp16 gates" not in bvar, (var, bvar)
    P, (lg, vl, am), _, diag = _oracle(T, B, mask, oracle_masks(agent.relu_trace, B), H, W)
    Gl, Gv = _cot(T, B)
    ((lg * Gl).sum() + (vl * Gv).sum()).backward()
    _compare(out, (lg.detach(), vl.detach(), am.detach(), reset_ref.grads(P), diag), BF16_RTOL, f"bf16 resets {case}: ")
    assert N.pair_status(clear=True) == 0


@pytest.mark.parametrize("path", ["frames", "steps"])
def test_segment_equivalence(cuda, monkeypatch, path):
    """(c) reset[s][:] = 1: one unroll of T steps against two plain bf16 unrolls of s and T-s steps from
    reset().  The recurrence runs the same instruction sequence on the same operands, so the outputs are
    expected to be equal; they are held to 1e-5, the figure test_gpu_resets.py uses.

    B = 5 keeps every segment above 8 frames, so the segments' tail GEMMs run the tiles the whole unroll runs.
    At B = 3 the first segment has 6 frames and takes the skinny tail kernels (plain fp32 FMAs) where the
    unroll of 15 frames takes the split-product tiles: the attention maps, hence every h_t, were still
    bit-identical, the logits differed by 9e-8, and that fp32 difference in the readout's cotangent reached
    the vision gradients through the backward's three bf16 roundings (dZ, dx, dY1) as 1.9e-4 (conv1 weight),
    7.8e-5 (conv2 weight), 6.7e-5 (W_ho) -- a property of the tail dispatch, with or without a mask."""
    _setenv(monkeypatch, HIP_ENV[path])
    T, B, s = 5, 5, 2
    X = _frames(T, B)
    Gl, Gv = _cot(T, B)
    agent = _agent(cuda)
    bound, _ = _spread_bound(agent, X, cuda)
    one, var, bvar = _timed(lambda: _run(agent, X, _mask(T, B, [(s, b) for b in range(B)]), cuda))
    assert var.endswith(", resets") and bvar.endswith(", resets") and ("k_convlstm_fwd_frames" in var) == (path == "frames")
    assert ("k_convlstm_bwd_frames" in bvar) == (path == "frames"), bvar
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
        want = torch.cat([parts[0][i], parts[1][i]])
        print(f"{path} segments {n}: max abs diff {float((one[i] - want).abs().max()):.3e}")
        assert_close(one[i].numpy(), want.numpy(), 1e-5, f"{path} segments {n}")
    _grads_close(one[3], two, bound, f"{path} segments")
    assert N.pair_status(clear=True) == 0


@pytest.mark.parametrize("path", ["frames", "steps"])
def test_frames_before_a_reset_reach_nothing_after_it(cuda, monkeypatch, path):
    """(d)"""
    _setenv(monkeypatch, HIP_ENV[path])
    T, B = 5, 4
    mask = _mask(T, B, MASK54)
    agent = _agent(cuda)
    X = _frames(T, B)
    a = _run(agent, X, mask, cuda)
    Y = X.clone()
    Y[:2, 1] = torch.from_numpy(detinit.frames_u8(99, (2, 84, 84, 3)).astype(np.float32))   # row 1 resets at t = 2
    b = _run(agent, Y, mask, cuda)
    for i, n in enumerate(("logits", "values", "attn")):
        assert torch.equal(a[i][2:, 1], b[i][2:, 1]), f"{path}: row 1 {n} after its reset"
        assert not torch.equal(a[i][:2, 1], b[i][:2, 1])
    assert N.pair_status(clear=True) == 0


def _state(B, nan_row, dev, seed):
    """A carried ConvLSTM state in the agent's (B, 128, w, h) layout, one row NaN."""
    s = torch.from_numpy(detinit.cotangent(seed, (B, 128, 11, 11))).clone()
    s[nan_row] = float("nan")
    return s.to(dev).requires_grad_()


@pytest.mark.parametrize("path", ["frames", "steps"])
def test_nan_state_under_a_reset(cuda, monkeypatch, path):
    """(e) a NaN row in the carried h0 / c0 under reset[0]: finite outputs equal to the zero-state run's, that
    row's state cotangents exactly 0."""
    _setenv(monkeypatch, HIP_ENV[path])
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

    nan = run(_state(B, row, cuda, 41), _state(B, row, cuda, 42), _mask(T, B, [(0, row), (2, 0)]).to(cuda))
    # the zero-state run: zeros in that row, no reset at its step 0
    hz, cz = (torch.nan_to_num(_state(B, row, cuda, k).detach(), nan=0.0).requires_grad_() for k in (41, 42))
    zero = run(hz, cz, _mask(T, B, [(2, 0)]).to(cuda))
    for i, n in enumerate(("logits", "values", "attn")):
        assert bool(torch.isfinite(nan[i]).all()) and torch.equal(nan[i], zero[i]), n
    for g in nan[3:]:
        assert bool(torch.isfinite(g).all()) and float(g[row].abs().max()) == 0.0
        assert float(g[2].abs().max()) > 0.0   # a row that read its state
    assert N.pair_status(clear=True) == 0


@pytest.mark.parametrize("path", ["frames", "steps"])
def test_all_zero_mask_is_no_mask(cuda, monkeypatch, path):
    """(f) the forward is bit-identical to reset=None on the same flagged agent (the same operations in the
    same order; the readout reads the HR copy of the same bf16 values); the gradients agree at (c)'s bound."""
    _setenv(monkeypatch, HIP_ENV[path])
    T, B = 4, 3
    agent = _agent(cuda)
    bound, none = _spread_bound(agent, _frames(T, B), cuda)
    zero = _run(agent, _frames(T, B), torch.zeros(T, B), cuda)
    for i, n in enumerate(("logits", "values", "attn")):
        assert torch.equal(none[i], zero[i]), f"{path}: zero mask moved {n}"
    _grads_close(zero[3], none[3], bound, f"{path} zero mask")
    assert N.pair_status(clear=True) == 0


@pytest.mark.parametrize("env", [FRAMES, {"AAA_FRAMES_FWD": "0"}], ids=["frames", "steps"])
def test_flagged_runner_without_a_mask_is_the_unflagged_runner(cuda, monkeypatch, env):
    """(g) the variant strings and the outputs, bit for bit (frames: the frame-resident forward and BPTT)."""
    _setenv(monkeypatch, env)
    T, B = 3, 4
    X = _frames(T, B)
    got = {}
    for resets in (False, True):
        agent = _agent(cuda, resets=resets)
        r = agent._runner(B, T, 84, 84, cuda)
        assert r.resets == resets and bool(r.cfg.flags & N.FLAG_BF16_RESETS) == resets
        got[resets] = _timed(lambda: _run(agent, X, None, cuda))
    (a, va, ba), (b, vb, bb) = got[False], got[True]
    assert va == vb and ba == bb and "resets" not in va + ba, (va, vb, ba, bb)
    if env is FRAMES:
        assert "k_convlstm_fwd_frames" in va and "k_convlstm_bwd_frames" in ba, (va, ba)
    for i, n in enumerate(("logits", "values", "attn")):
        assert torch.equal(a[i], b[i]), n
    assert N.pair_status(clear=True) == 0


def test_unflagged_agent_names_the_keyword(cuda):
    agent = _agent(cuda, resets=False)
    with pytest.raises(RuntimeError, match="resets=True"):
        agent.unroll(_frames(2, 2).to(cuda), reset=torch.zeros(2, 2, device=cuda))
    r = UnrollRunner(2, 2, 84, 84, dtype="bf16", device=cuda)
    flat = torch.cat([p.detach().reshape(-1) for p in agent.parameters()])
    packed, ws = r.new_packed(), r.new_workspace()
    r.pack(flat, packed)
    with pytest.raises(RuntimeError, match="AAA_FLAG_BF16_RESETS"):
        r.forward(flat, packed, agent.spatial.S.to(cuda).contiguous(), _frames(2, 2).to(cuda), ws,
                  reset=torch.zeros(2, 2, device=cuda))
    assert N.pair_status(clear=True) == 0


def test_stateful_core_vs_bf16_oracle(cuda, monkeypatch):
    """The stateful core under a mask (its reset handling works on fp32 buffers; the readout reads HR): core
    state carried in and out, core_h0 NaN in a row with reset[0]; the mask of test_gpu_resets.py's
    test_stateful_core_vs_reference."""
    _setenv(monkeypatch, FRAMES)
    T, B = 5, 3
    mask = _mask(T, B, ((0, 1), (2, 0), (3, 0), (4, 2)))
    ch = torch.from_numpy(detinit.cotangent(51, (B, 256))).clone()
    cc = torch.from_numpy(detinit.cotangent(52, (B, 256))).clone()
    Gc = torch.from_numpy(detinit.cotangent(53, (B, 256)))
    Gl, Gv = _cot(T, B)

    agent = _agent(cuda, stateful=True)
    agent.relu_trace = []
    agent.reset()
    h0 = ch.clone()
    h0[1] = float("nan")   # row 1 starts an episode at step 0: never read
    h0, c0 = h0.to(cuda).requires_grad_(), cc.to(cuda).requires_grad_()
    agent.prev_output, agent.prev_hidden = h0, c0

    def go():
        lg, vl, am = agent.unroll(_frames(T, B).to(cuda), reset=mask.to(cuda))
        g = Gc.to(cuda)
        ((lg * Gl.to(cuda)).sum() + (vl * Gv.to(cuda)).sum() + (agent.prev_output * g).sum()
         + (agent.prev_hidden * g).sum()).backward()
        torch.cuda.synchronize()
        return lg.detach().cpu(), vl.detach().cpu(), am.detach().cpu(), _grads(agent)

    out, var, bvar = _timed(go)
    assert "k_convlstm_fwd_frames" in var and var.endswith(", resets"), var
    assert "k_convlstm_bwd_frames" in bvar and bvar.endswith(", resets"), bvar
    assert all(bool(torch.isfinite(o).all()) for o in out[:3])
    nan_grads = (h0.grad.cpu().clone(), c0.grad.cpu().clone())
    core_out = (agent.prev_output.detach().cpu().clone(), agent.prev_hidden.detach().cpu().clone())
    # the zero-state run: zeros in row 1 of core_h0, the same mask -- the select makes them the same computation
    agent.reset()
    agent.zero_grad()
    hz = ch.clone()
    hz[1] = 0.0
    hz, cz = hz.to(cuda).requires_grad_(), cc.to(cuda).requires_grad_()
    agent.prev_output, agent.prev_hidden = hz, cz
    zero = go()
    for i, n in enumerate(("logits", "values", "attn")):
        assert torch.equal(out[i], zero[i]), f"NaN core_h0 under reset[0]: {n} differs from the zero-state run"
    assert torch.equal(core_out[0], agent.prev_output.detach().cpu()) and torch.equal(core_out[1], agent.prev_hidden.detach().cpu())
    for a, b, n in zip(nan_grads, (hz.grad.cpu(), cz.grad.cpu()), ("dcore_h0", "dcore_c0")):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), n
    agent.relu_trace = agent.relu_trace[:1]   # the first run's masks, for the oracle

    rch, rcc = ch.clone().requires_grad_(), cc.clone().requires_grad_()
    P, (rl, rv, ra), (_, rcore), diag = _oracle(T, B, mask, oracle_masks(agent.relu_trace, B, stateful=True),
                                                core_state=(rch, rcc), stateful_core=True)
    ((rl * Gl).sum() + (rv * Gv).sum() + (rcore[0] * Gc).sum() + (rcore[1] * Gc).sum()).backward()
    _compare(out, (rl.detach(), rv.detach(), ra.detach(), reset_ref.grads(P), diag), BF16_RTOL, "bf16 stateful resets: ")
    assert_close(agent.prev_output.detach().cpu().numpy(), rcore[0].detach().numpy(), BF16_RTOL, "core hT")
    assert_close(agent.prev_hidden.detach().cpu().numpy(), rcore[1].detach().numpy(), BF16_RTOL, "core cT")
    for got, want, n in ((h0.grad, rch.grad, "dcore_h0"), (c0.grad, rcc.grad, "dcore_c0")):
        assert float(got[1].abs().max()) == 0.0, n
        assert_close(got.cpu().numpy(), want.numpy(), BF16_RTOL, n)
    assert N.pair_status(clear=True) == 0


def test_learner_reset_done(cuda, monkeypatch):
    """(h) Learner(dtype="bf16", resets=True): reset="done" is the explicit episode_starts mask, differs from
    reset=None after the first done, train_on passes the mask of a recorded unroll; an unflagged bf16 learner
    behaves as before."""
    from aaa_amd.learner import Learner
    from aaa_amd.unroll import Unroll
    _setenv(monkeypatch, FRAMES)
    T, B = 5, 3
    frames = _frames(T, B).to(cuda).contiguous()
    actions = torch.from_numpy((detinit.frames_u8(7, (T, B)) % 18).astype(np.int32)).to(cuda)
    rewards = torch.from_numpy(detinit.cotangent(8, (T, B))).to(cuda)
    blogp = -torch.from_numpy(detinit.cotangent(9, (T, B))).abs().to(cuda)
    done = _mask(T, B, [(1, 0), (3, 2)]).to(cuda)

    def step(resets=True, **kw):
        lr = Learner(B=B, T=T, dtype="bf16", device=cuda, resets=resets)
        (lg, _, _), _, bvar = _timed(lambda: lr.train_step_vtrace(frames, actions, rewards, blogp, done, "last", **kw))
        torch.cuda.synchronize()
        lr.check_health()
        return lg.cpu(), lr.grads.cpu().clone(), bvar

    by_name = step(reset="done")
    explicit = step(reset=episode_starts(done))
    none = step()
    plain = step(resets=False)
    assert by_name[2].endswith(", resets") and "resets" not in none[2]
    assert torch.equal(by_name[0], explicit[0])
    # two runs of the same launches: atomic sums (test_gpu_parity.py test_repeat_is_deterministic_enough: 1e-5)
    spread = rel_err(none[1].numpy(), plain[1].numpy())
    print(f"learner: plain repeat spread {spread:.3e}")
    assert torch.equal(none[0], plain[0]) and none[2] == plain[2]
    assert rel_err(by_name[1].numpy(), explicit[1].numpy()) <= max(1e-5, 4 * spread)
    # done at (1, 0) and (3, 2): steps 0-1 are reset=None's, row 0 from step 2 on is not
    assert torch.equal(by_name[0][:2], none[0][:2])
    assert not torch.equal(by_name[0][2:, 0], none[0][2:, 0])
    assert rel_err(by_name[1].numpy(), none[1].numpy()) > 1e-3
    with pytest.raises(RuntimeError, match="AAA_FLAG_BF16_RESETS"):
        step(resets=False, reset="done")

    # train_on: a recorded unroll with a done inside passes the mask on a flagged learner, none on an unflagged one
    u = Unroll(frames.to(torch.uint8), actions, rewards * (1 - _mask(T, B, [(T - 1, b) for b in range(B)]).to(cuda)),
               blogp, done * (1 - _mask(T, B, [(T - 1, b) for b in range(B)]).to(cuda)), torch.zeros(B, device=cuda),
               (torch.zeros(B, 11, 11, 128, device=cuda), torch.zeros(B, 11, 11, 128, device=cuda)))
    for resets in (True, False):
        lr = Learner(B=B, T=T, dtype="bf16", device=cuda, resets=resets, frames_u8=True)
        _, var, bvar = _timed(lambda: lr.train_on(u))
        torch.cuda.synchronize()
        lr.check_health()
        assert var.endswith(", resets") == resets and bvar.endswith(", resets") == resets, (resets, var, bvar)
    assert N.pair_status(clear=True) == 0
