"""Gradient clipping by global norm on the device (csrc/optim.hip k_gradsq /
k_gradsq_finish / k_grad_scale / k_adam<clip>; include/aaa.h aaa_grad_norm,
aaa_grad_scale, aaa_adam_step_clipped) against its float64 statement
(tests/clip_ref.py, itself checked on the CPU by tests/test_clip_emulation.py).

Tolerances.  The norm: 1 fp32 ulp from the fp32 rounding of the reference
norm -- derived, not tuned: the kernel sums exact squares in double, so any
order is within N * 2^-53 ~ 2.5e-10 relative of the exact sum, far inside half
an fp32 ulp, and the rounding to fp32 can then differ by one step at most.
The coefficient: 1 ulp likewise.  Adam: the project's existing 1e-6 relative
to max|.| (tests/test_gpu_optim.py), with the reference fed the device's own
coefficient (pinned within 1 ulp here)."""
import functools
import json
import math
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from helpers import ROOT, assert_close, detinit

import attention  # noqa: F401
import clip_ref as C
import vtrace_ref as R
from aaa_amd import _native as N
from aaa_amd.optim import Adam, adam_flat_, clip_grad_norm_

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
FLAT = 2_270_276


def _shapes():
    # the 34 reference tensors plus odd sizes (vector tail, scalar path), as tests/test_gpu_optim.py
    return [tuple(v.shape) for v in detinit.deterministic_params(0, 18, 4).values()] + [(1,), (3,), (1025,), (7, 9)]


def _randn(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * (10.0 ** (i % 3 - 1)) for i, s in enumerate(shapes)]


FIFTY = [(1 + (i * 37) % 300,) for i in range(49)] + [(C.CHUNK + 5,)]   # two kernel tables (48 + 2)


@functools.lru_cache(maxsize=None)
def _list(name):
    """CPU gradient lists, computed once and shared (read-only).  "edge": tensor 3 is put
    4 bytes off 16-byte alignment on the device (_to_dev): the scalar path."""
    shapes = {"shapes": _shapes(), "edge": [(0,), (C.CHUNK,), (C.CHUNK + 1,), (1025,), (2 * C.CHUNK + 7,)],
              "fifty": FIFTY, "flat": [(FLAT,)]}[name]
    return tuple(_randn(shapes, 5 + len(shapes)))


@functools.lru_cache(maxsize=None)
def _norm(name):
    return C.norm64(_list(name))


def _to_dev(ts, dev, misalign=()):
    out = []
    for i, t in enumerate(ts):
        if i in misalign:
            buf = torch.empty(t.numel() + 1, device=dev)
            v = buf[1:].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
            out.append(v)
        else:
            out.append(t.to(dev))
    return out


def _scratch(ts, dev, fill=None):
    s = torch.empty(N.grad_norm_scratch_bytes([t.numel() for t in ts]) // 8, dtype=torch.float64, device=dev)
    if fill is not None:
        s.fill_(fill)
    return s


def _stats(gs, max_norm, dev, fill=None):
    stats = torch.full((4,), NAN, device=dev)
    N.grad_norm(max_norm, gs, stats, _scratch(gs, dev, fill))
    torch.cuda.synchronize()
    return stats.cpu().numpy()


def _check_stats(s, ref, what):
    """Device stats against the reference within the derived tolerance (module docstring)."""
    r = ref["stats"]
    print(f"{what}: norm {s[0]!r} (ref {r[0]!r}), coef {s[1]!r} (ref {r[1]!r}), flag {s[2]}")
    for k in (0, 1):
        if np.isfinite(r[k]):
            assert np.isfinite(s[k]) and C.ulps(s[k], r[k]) <= 1, (what, k, s[k], r[k])
        else:
            assert C.same_f32(s[k], r[k]), (what, k, s[k], r[k])
    assert s[2] == np.float32(ref["nonfinite"]) and C.same_f32(s[3], r[3]), (what, s)


@pytest.mark.parametrize("name", ["shapes", "edge", "fifty", "flat"])
def test_norm_and_coefficient(cuda, name):
    cpu = _list(name)
    gs = _to_dev(cpu, cuda, misalign=(3,) if name == "edge" else ())
    n = _norm(name)
    for max_norm in (0.5 * n, n, 2.0 * n, INF, 1e-30):
        ref = C.reference(cpu, max_norm, norm=n)
        s = _stats(gs, max_norm, cuda)
        _check_stats(s, ref, f"{name} max_norm={max_norm:.6g}")
        if n * (1.0 + 2.0 ** -23) + 1e-6 < max_norm:   # below the limit by more than the norm's ulp: not clipped
            assert s[1] == np.float32(1.0)
        if max_norm <= 0.5 * n:
            assert s[1] < np.float32(1.0)
        # the same input again, over a scratch full of NaN: bit-identical (fixed order, no stale partial read)
        s2 = _stats(gs, max_norm, cuda, fill=NAN)
        assert s.tobytes() == s2.tobytes(), (name, s, s2)


def test_empty_inputs(cuda):
    for gs in ([], [torch.empty(0, device=cuda)], [torch.empty(0, device=cuda)] * 3):
        stats = torch.full((4,), NAN, device=cuda)
        N.grad_norm(2.5, gs, stats, torch.full((2,), NAN, dtype=torch.float64, device=cuda))
        N.grad_scale(stats, gs)
        torch.cuda.synchronize()
        assert stats.tolist() == [0.0, 1.0, 0.0, 2.5]


# ---------------------------------------------------------------- non-finite ---
def _plant(gs, where, value):
    gs = [g.clone() for g in gs]
    for (t, i), v in zip(where, value):
        gs[t].view(-1)[i] = v
    return gs


_rng = np.random.default_rng(7)
_T0 = int(_rng.integers(0, 48))
NONFINITE = {
    "nan at a seeded index": ([(_T0, int(_rng.integers(0, FIFTY[_T0][0])))], [NAN]),
    "nan at the last element of the last tensor": ([(49, FIFTY[49][0] - 1)], [NAN]),
    "nan in the 49th tensor": ([(48, 0)], [NAN]),
    "+inf": ([(7, 3)], [INF]),
    "+inf and -inf": ([(7, 3), (49, C.CHUNK + 1)], [INF, -INF]),
}


@pytest.mark.parametrize("what", sorted(NONFINITE))
def test_nonfinite_step_is_skipped_and_not_counted(cuda, what):
    """Finite step, non-finite step, finite step: the middle one leaves params, both
    moments and the device step counter bit-identical, and the last applies as update 2."""
    where, value = NONFINITE[what]
    g = torch.Generator().manual_seed(21)
    p0 = [torch.randn(s, generator=g) for s in FIFTY]
    steps = [_randn(FIFTY, 31), _plant(_randn(FIFTY, 32), where, value), _randn(FIFTY, 33)]
    ps = _to_dev(p0, cuda)
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    step_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
    guard = torch.zeros(1, device=cuda)
    hp = N.AdamHP(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)
    coefs = []
    for k, gs_cpu in enumerate(steps):
        gs = _to_dev(gs_cpu, cuda)
        before = [t.clone() for t in ps + ms + vs]
        s = _stats(gs, 1.0, cuda)
        stats = torch.from_numpy(s).to(cuda)
        N.adam_step(hp, 0, ps, gs, ms, vs, guard=guard, step_dev=step_dev, clip=stats)
        torch.cuda.synchronize()
        if k == 1:
            _check_stats(s, C.reference(gs_cpu, 1.0), what)
            assert s[2] == 1.0
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, ps + ms + vs))
            assert int(step_dev.item()) == 1
            coefs.append(None)
        else:
            assert s[2] == 0.0 and int(step_dev.item()) == (1 if k == 0 else 2)
            coefs.append(s[1])
    rp, rm, rv = C.clipped_adam_reference(p0, steps, coefs, lr=1e-3)
    _close(ps, rp, "param")
    _close(ms, rm, "exp_avg")
    _close(vs, rv, "exp_avg_sq")


def _close(dut, ref, what, tol=1e-6):
    """The project's Adam tolerance: 1e-6 relative to max|.| of each tensor."""
    for i, (a, b) in enumerate(zip(dut, ref)):
        a, b = a.detach().cpu().double(), b.detach().double()
        if b.numel() == 0:
            continue
        assert bool(torch.isfinite(a).all()), (what, i)
        err = float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))
        assert err < tol, (what, i, err)


# ------------------------------------------------------------------- drop-in ---
@pytest.mark.parametrize("name", ["shapes", "fifty"])
def test_clip_grad_norm_drop_in(cuda, name):
    cpu = _list(name)
    n = _norm(name)
    g = torch.Generator().manual_seed(3)
    p0 = [torch.randn(t.shape, generator=g) for t in cpu]
    ps = [torch.nn.Parameter(p.clone().to(cuda)) for p in p0]
    for p, t in zip(ps, cpu):
        p.grad = t.clone().to(cuda)
    # not clipped: the gradients are untouched bit for bit
    stats = torch.full((4,), NAN, device=cuda)
    ret = clip_grad_norm_(ps, 2.0 * n, stats=stats)
    torch.cuda.synchronize()
    assert float(stats[1]) == 1.0 and ret.dim() == 0 and ret.data_ptr() == stats.data_ptr()
    assert all(torch.equal(p.grad.cpu().view(torch.int32), t.view(torch.int32)) for p, t in zip(ps, cpu))
    # clipped: grad * coef, the fp32 multiply redone on the host with the coefficient the device wrote
    ret = clip_grad_norm_(ps, 0.5 * n, stats=stats)
    torch.cuda.synchronize()
    s = stats.cpu().numpy()
    _check_stats(s, C.reference(cpu, 0.5 * n), name)
    assert s[1] < 1.0 and float(ret) == float(s[0])
    coef = torch.tensor(float(s[1]), dtype=torch.float32)
    for i, (p, t) in enumerate(zip(ps, cpu)):
        assert torch.equal(p.grad.cpu().view(torch.int32), (t * coef).view(torch.int32)), i
    # without stats=: the 0-d device norm, as torch returns it
    again = clip_grad_norm_(ps, INF)
    assert again.is_cuda and again.dim() == 0 and float(again) > 0.0
    # then the fused Adam on the clipped gradients, against the reference path
    Adam(ps, lr=1e-3).step()
    torch.cuda.synchronize()
    rp, _, _ = C.clipped_adam_reference(p0, [list(cpu)], [s[1]], lr=1e-3)
    _close(ps, rp, "param after clip + Adam.step")
    # error_if_nonfinite reads the flag
    ps[1].grad.view(-1)[0] = NAN
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)
    with pytest.raises(ValueError):
        clip_grad_norm_(ps, 1.0, norm_type=INF)


# -------------------------------------------------------------- clipped Adam ---
@pytest.mark.parametrize("kw", [dict(lr=1e-3), dict(lr=3e-3, weight_decay=0.01)])
def test_clipped_adam_matches_reference(cuda, kw):
    shapes = _shapes()
    g = torch.Generator().manual_seed(5)
    p0 = [torch.randn(s, generator=g) for s in shapes]
    steps = [[t * (4.0 if k % 2 == 0 else 1.0) for t in _randn(shapes, 40 + k)] for k in range(4)]
    for gs in steps:      # exactly-zero gradients stay part of the picture (tests/test_gpu_optim.py)
        gs[27].zero_()
    norms = [C.norm64(gs) for gs in steps]
    max_norm = math.sqrt(min(norms[0], norms[2]) * max(norms[1], norms[3]))   # steps 1 and 3 clip, 2 and 4 do not
    assert max(norms[1], norms[3]) * 1.5 < max_norm < min(norms[0], norms[2]) / 1.5
    ps = _to_dev(p0, cuda)
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    step_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
    guard = torch.zeros(1, device=cuda)
    hp = N.AdamHP(kw["lr"], 0.9, 0.999, 1e-8, kw.get("weight_decay", 0.0), 0, 0)
    stats = torch.full((4,), NAN, device=cuda)
    coefs = []
    for k, gs_cpu in enumerate(steps):
        gs = _to_dev(gs_cpu, cuda)
        N.grad_norm(max_norm, gs, stats, _scratch(gs, cuda))
        N.adam_step(hp, 0, ps, gs, ms, vs, guard=guard, step_dev=step_dev, clip=stats)
        torch.cuda.synchronize()
        s = stats.cpu().numpy()
        _check_stats(s, C.reference(gs_cpu, max_norm), f"step {k + 1}")
        assert (s[1] < 1.0) if k % 2 == 0 else (s[1] == 1.0), (k, s)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(gs, gs_cpu))   # the gradients themselves are not written
        coefs.append(s[1])
    assert int(step_dev.item()) == 4
    rp, rm, rv = C.clipped_adam_reference(p0, steps, coefs, **kw)
    _close(ps, rp, "param")
    _close(ms, rm, "exp_avg")
    _close(vs, rv, "exp_avg_sq")
    # a non-zero guard with finite stats also skips
    before = [t.clone() for t in ps + ms + vs]
    guard.fill_(1.0)
    N.adam_step(hp, 0, ps, _to_dev(steps[0], cuda), ms, vs, guard=guard, step_dev=step_dev, clip=stats)
    torch.cuda.synchronize()
    assert float(stats[2]) == 0.0 and int(step_dev.item()) == 4
    assert all(torch.equal(a, b) for a, b in zip(before, ps + ms + vs))


def test_unclipped_step_is_bit_identical_to_the_counted_adam(cuda):
    """weight_decay = 0 and a coefficient of exactly 1 on every step: adam_flat_ with
    clip= gives what adam_flat_ without it gives, with the same guard and step_dev."""
    n = 3 * C.CHUNK + 5
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, generator=g)
    state = []
    for clip in (False, True):
        p, m, v = p0.clone().to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
        step_dev, guard = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(1, device=cuda)
        stats = torch.full((4,), NAN, device=cuda)
        gg = torch.Generator().manual_seed(10)
        for _ in range(3):
            gr = torch.randn(n, generator=gg).to(cuda)
            if clip:
                N.grad_norm(INF, [gr], stats, _scratch([gr], cuda))
            adam_flat_(p, gr, m, v, 0, lr=1e-3, guard=guard, step_dev=step_dev, clip=stats if clip else None)
        torch.cuda.synchronize()
        if clip:
            assert float(stats[1]) == 1.0 and float(stats[2]) == 0.0 and math.isinf(float(stats[3]))
        state.append((p, m, v, step_dev))
    for a, b in zip(*state):
        assert torch.equal(a, b)
    assert int(state[1][3].item()) == 3


def test_clipped_adam_without_a_guard(cuda):
    """guard = NULL (include/aaa.h): the clipped update then depends on the stats alone -- bit for
    bit what a zero guard gives on a clipped step, and a non-finite norm still skips."""
    n = 2 * C.CHUNK + 3
    g = torch.Generator().manual_seed(12)
    p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g).to(cuda)
    stats = torch.full((4,), NAN, device=cuda)
    N.grad_norm(0.5 * C.norm64([gr.cpu()]), [gr], stats, _scratch([gr], cuda))
    state = []
    for guard in (torch.zeros(1, device=cuda), None):
        p, m, v = p0.clone().to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
        step_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
        adam_flat_(p, gr, m, v, 0, lr=1e-3, guard=guard, step_dev=step_dev, clip=stats)
        torch.cuda.synchronize()
        state.append((p, m, v, step_dev))
    assert 0.0 < float(stats[1]) < 1.0 and float(stats[2]) == 0.0
    for a, b in zip(*state):
        assert torch.equal(a, b)
    p, m, v, step_dev = state[1]
    assert int(step_dev.item()) == 1 and not torch.equal(p.cpu(), p0)
    before = [t.clone() for t in (p, m, v)]
    bad = gr.clone()
    bad[n - 1] = NAN
    N.grad_norm(1.0, [bad], stats, _scratch([bad], cuda))
    adam_flat_(p, bad, m, v, 0, lr=1e-3, guard=None, step_dev=step_dev, clip=stats)
    torch.cuda.synchronize()
    assert float(stats[2]) == 1.0 and int(step_dev.item()) == 1
    assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v)))


# ------------------------------------------------------------------- learner ---
AG_A = 18
AG_HP = dict(gamma=0.97, lam=0.9, rho_bar=1.3, c_bar=0.8, pg_rho_bar=2.0, baseline_cost=0.5, entropy_cost=0.01)


def _agent_inputs(T, B):
    """The inputs of tests/test_gpu_vtrace.py's learner test, rebuilt here."""
    x = R.make_inputs(T, B, AG_A, 23)
    x["done"][:] = 0
    x["done"][1, 0] = 1.0
    frames = torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3)).astype(np.float32))
    return frames, {k: x[k] for k in ("actions", "rewards", "behaviour_logp", "done", "bootstrap")}


def _host_reads(fn):
    """The host-read names a function's code (nested functions included) touches."""
    banned = {"item", "cpu", "tolist", "numpy", "synchronize", "nonzero"}
    code = fn.__code__ if hasattr(fn, "__code__") else fn
    hits = banned & set(code.co_names)
    for c in code.co_consts:
        if hasattr(c, "co_names"):
            hits |= _host_reads(c)
    return hits


def test_learner_clips_and_skips(cuda):
    from aaa_amd.learner import Learner
    T, B = 3, 2
    hp = dict(AG_HP, scale=1.0 / (T * B))
    frames, x = _agent_inputs(T, B)
    frames = frames.to(cuda).contiguous()
    d = {k: v.to(cuda) for k, v in x.items()}
    # max_grad_norm=None is the learner as it was.  The small-batch backward accumulates its split-K
    # weight gradients with floating-point atomics (csrc/epilogues.h), so two runs of the same
    # iteration differ in the gradients' last bits whatever the optimizer does: the two learners'
    # gradients are compared as the existing learner test compares them (1e-6), and each learner's
    # parameters and moments bit for bit with the counted Adam as it was, replayed on that learner's
    # own gradients from the same start.
    plain, none = Learner(B=B, T=T, device=cuda), Learner(B=B, T=T, device=cuda, max_grad_norm=None)
    start = plain.flat.clone()
    assert torch.equal(start, none.flat)
    for ln in (plain, none):
        ln.train_step_vtrace(frames, **d, **hp)
    torch.cuda.synchronize()
    differing = int((plain.grads != none.grads).sum())
    print(f"gradient elements that differ between two runs of one iteration: {differing} of {plain.grads.numel()}, "
          f"max |diff| {float((plain.grads - none.grads).abs().max()):.3e}; parameters equal: "
          f"{torch.equal(plain.flat, none.flat)}")
    assert_close(none.grads.cpu().numpy(), plain.grads.cpu().numpy(), 1e-6, "grads with max_grad_norm=None")
    for ln in (plain, none):
        p, m, v = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
        sd = torch.zeros(1, dtype=torch.int32, device=cuda)
        adam_flat_(p, ln.grads, m, v, 0, lr=ln.lr, guard=ln.guard, step_dev=sd)
        torch.cuda.synchronize()
        assert torch.equal(ln.flat, p) and torch.equal(ln.exp_avg, m) and torch.equal(ln.exp_avg_sq, v)
        assert ln.opt_steps == 1 and ln.grad_stats.tolist() == [0.0] * 4   # no clip launch wrote the stats
    n0 = C.norm64([plain.grads.cpu()])
    assert math.isfinite(n0) and n0 > 0.0
    # half the norm that learner's gradients had: a clipped iteration, with no host read in it
    lr = Learner(B=B, T=T, device=cuda, max_grad_norm=0.5 * n0)
    before = lr.flat.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("error")
    try:
        lr.train_step_vtrace(frames, **d, **hp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert not _host_reads(Learner.optimizer_step), _host_reads(Learner.optimizer_step)
    rep = lr.clip_report()
    grads = lr.grads.cpu()
    assert C.ulps(rep["norm"], np.float32(C.norm64([grads]))) <= 1
    assert 0.0 < rep["coef"] < 1.0 and rep["nonfinite"] == 0 and rep["max_norm"] == float(np.float32(0.5 * n0))
    assert lr.opt_steps == 1
    rp, rm, rv = C.clipped_adam_reference([before.cpu()], [[grads]], [rep["coef"]], lr=1e-3)
    _close([lr.flat], rp, "flat")
    _close([lr.exp_avg], rm, "exp_avg")
    _close([lr.exp_avg_sq], rv, "exp_avg_sq")
    # an action of value A in one row: NaN cotangents, NaN gradients -- the step is skipped, nothing stranded
    state = [t.clone() for t in (lr.flat, lr.exp_avg, lr.exp_avg_sq)]
    bad = dict(d, actions=d["actions"].clone())
    bad["actions"][1, 0] = AG_A
    lr.train_step_vtrace(frames, **bad, **hp)
    torch.cuda.synchronize()
    assert bool(torch.isnan(lr.grads).any())
    assert all(torch.equal(a, b) for a, b in zip(state, (lr.flat, lr.exp_avg, lr.exp_avg_sq)))
    assert lr.opt_steps == 1 and lr.clip_report()["nonfinite"] == 1
    lr.check_health()
    lr.train_step_vtrace(frames, **d, **hp)
    torch.cuda.synchronize()
    assert lr.opt_steps == 2 and lr.clip_report()["nonfinite"] == 0
    assert not torch.equal(lr.flat, state[0]) and bool(torch.isfinite(lr.flat).all())
    lr.check_health()


# ------------------------------------------------------------------------ DP ---
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_dp_ranks_clip_and_skip_alike():
    """tools/dp_clip_check.py: 2 ranks on cuda:0 over gloo, B = 2 per rank, T = 3."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(ROOT, "tools", "dp_clip_check.py")]
    env = dict(os.environ, AAA_DP_BACKEND="gloo", OMP_NUM_THREADS="2", AAA_DP_B="2", AAA_DP_T="3")
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1])
    print(res)
    assert res["world"] == 2
    assert res["clipped_stats_identical"] and res["norm_ulps_worst_rank"] <= 1 and res["coef_below_one"]
    assert res["flat_identical_after_clipped_step"] and res["opt_steps_after_clipped_step"] == [1, 1]
    assert res["nonfinite_flag_per_rank"] == [1.0, 1.0] and res["flat_unchanged_on_every_rank"]
    assert res["opt_steps_after_skipped_step"] == [1, 1] and res["flat_identical_after_skipped_step"]
    assert res["health_after_skipped_step"] == "quiet"
    assert res["clean_step_moved_every_rank"] and res["flat_identical_after_clean_step"]
    assert res["opt_steps_after_clean_step"] == [2, 2] and res["stats_identical_after_clean_step"]
    assert res["ok"]
