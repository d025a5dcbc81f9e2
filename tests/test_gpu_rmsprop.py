"""The fused RMSProp (csrc/optim.hip k_rmsprop; include/aaa.h aaa_rmsprop_step;
aaa_amd.optim.RMSprop / rmsprop_flat_; Learner(optimizer="rmsprop")) against its
float64 statement (tests/rmsprop_ref.py, itself checked on the CPU against
torch.optim.RMSprop by tests/test_rmsprop_emulation.py).

Tolerance.  The error of a tensor is max |got - ref| over max |ref|, for the
parameters and for every state tensor.  It may be at most the larger of
  1e-6, the project's optimizer tolerance (tests/test_gpu_optim.py), and
  twice the distance of torch.optim.RMSprop(foreach=False) in fp32 on the CPU
  from the same statement on the same inputs
-- the kernel evaluates torch's op order in fp32, and the centered variance
subtracts, so it is as good as the reference implementation and no better.
torch has no eps inside the square root, so the cases with ``eps_in_sqrt``
(IMPALA's, the learner's) have no second term: 1e-6 alone.  Both distances are
in every assertion message."""
import copy
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from helpers import ROOT, assert_close, detinit, rel_err  # noqa: F401

import attention  # noqa: F401
import clip_ref as C
import rmsprop_ref as R
import vtrace_ref as VR
from aaa_amd import _native as N
from aaa_amd.optim import RMSprop, adam_flat_, rmsprop_flat_, rmsprop_lr

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
TOL = 1e-6
STEPS = 6

# the 34 reference tensors, odd sizes (vector tail), one chunk (4096 elements) and its neighbours, an empty tensor
SHAPES = [tuple(v.shape) for v in detinit.deterministic_params(0, 18, 4).values()] + [
    (1,), (3,), (1025,), (7, 9), (4095,), (4096,), (4097,), (0,)]
OFFSET = 36     # (1025,): a view one element into its buffer on the device -- the all-scalar path
ZERO = 27       # its gradient is exactly zero on every step
assert SHAPES[OFFSET] == (1025,) and len(SHAPES) == 42

CASES = {
    "plain": dict(lr=1e-2),
    "impala": dict(lr=6e-4, alpha=0.99, eps=0.01, eps_in_sqrt=True),
    "weight_decay": dict(lr=3e-3, weight_decay=0.01),
    "momentum": dict(lr=1e-3, momentum=0.9),
    "centered": dict(lr=1e-3, centered=True),
    "centered + momentum": dict(lr=1e-3, centered=True, momentum=0.9),
    "maximize": dict(lr=1e-3, alpha=0.9, eps=1e-6, maximize=True),
}


@functools.lru_cache(maxsize=None)
def _inputs(shapes=None, seed=5, steps=STEPS):
    """(parameters, per-step gradients) on the CPU, computed once and shared (read-only): gradient
    magnitudes cycle over 0.1 / 1 / 10 with the step and the tensor."""
    shapes = SHAPES if shapes is None else list(shapes)
    g = torch.Generator().manual_seed(seed)
    ps = tuple(torch.randn(s, generator=g) for s in shapes)
    grads = tuple(tuple(torch.randn(s, generator=g) * (10.0 ** ((i + k) % 3 - 1)) for i, s in enumerate(shapes))
                  for k in range(steps))
    if shapes == SHAPES:
        for gs in grads:
            gs[ZERO].zero_()
    return ps, grads


@functools.lru_cache(maxsize=None)
def _reference(case):
    """The float64 statement and torch's fp32 CPU run of a parity case, once."""
    ps, grads = _inputs()
    hp = CASES[case]
    ref = R.run(ps, grads, **hp)
    t32 = None if hp.get("eps_in_sqrt") else R.torch_fp32(ps, grads, **hp)
    return ref, t32


def _to_dev(ts, dev, offset=()):
    out = []
    for i, t in enumerate(ts):
        if i in offset:
            buf = torch.empty(t.numel() + 1, device=dev)
            v = buf[1:].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
            out.append(v)
        else:
            out.append(t.to(dev))
    return out


def _check(got, ref, t32, what):
    """Every tensor of ``got`` within max(1e-6, 2 * torch's own fp32 distance) of ``ref`` (module docstring)."""
    worst = (0.0, None)
    for i, (a, b) in enumerate(zip(got, ref)):
        d = R.distance(a, b)
        d32 = R.distance(t32[i], b) if t32 is not None else None
        bound = max(TOL, 2.0 * d32) if d32 is not None else TOL
        worst = max(worst, (d, i))
        assert d <= bound, (f"{what}[{i}] {tuple(b.shape)}: kernel {d:.3e} from the float64 statement, torch fp32 CPU "
                            f"{'n/a (no eps_in_sqrt in torch)' if d32 is None else format(d32, '.3e')}, bound {bound:.3e}")
    print(f"{what}: worst {worst[0]:.3e} (tensor {worst[1]})")


def _check_all(ps, state, ref, t32, hp, what):
    _check(ps, ref["params"], t32 and t32["params"], f"{what} params")
    for k in R.used(dict(R.DEFAULTS, **hp)):
        _check(state[k], ref[k], t32 and t32[k], f"{what} {k}")


def _bits(ts):
    return [t.detach().clone().view(torch.int32) if t.numel() else t.detach().clone() for t in ts]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _hp(**kw):
    f = dict(R.DEFAULTS, **kw)
    return N.RmspropHP(f["lr"], f["alpha"], f["eps"], f["weight_decay"], f["momentum"], f["lr_end"], f["anneal_steps"],
                       int(f["centered"]), int(f["maximize"]), int(f["eps_in_sqrt"]))


def _state(ps, hp, offset=()):
    """Zero state on the device for the raw entry: (square_avg, momentum_buf or None, grad_avg or None)."""
    f = dict(R.DEFAULTS, **hp)
    def zeros():
        return _to_dev([torch.zeros(p.shape) for p in ps], ps[0].device, offset)
    return zeros(), (zeros() if f["momentum"] > 0 else None), (zeros() if f["centered"] else None)


def _scratch(ts, dev):
    return torch.empty(N.grad_norm_scratch_bytes([t.numel() for t in ts]) // 8, dtype=torch.float64, device=dev)


# -------------------------------------------------------------------- parity ---
@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_the_float64_statement(cuda, case):
    """Six steps of the drop-in optimizer over the 42 tensors, one of them on the scalar path."""
    hp = CASES[case]
    cpu, grads = _inputs()
    ref, t32 = _reference(case)
    dut = [torch.nn.Parameter(t) for t in _to_dev(cpu, cuda, offset=(OFFSET,))]
    assert dut[OFFSET].data_ptr() % 16 == 4
    opt = RMSprop(dut, **hp)
    versions = [p._version for p in dut]
    for gs in grads:
        for p, g in zip(dut, gs):
            p.grad = g.to(cuda)
        opt.step()
    torch.cuda.synchronize()
    full = dict(R.DEFAULTS, **hp)
    state = {k: [opt.state[p][k] for p in dut] for k in R.used(full)}
    _check_all(dut, state, ref, t32, hp, case)
    for p in dut:   # torch's state keys, and only the ones in use
        assert set(opt.state[p]) == {"step"} | set(R.used(full)) and float(opt.state[p]["step"]) == STEPS
    assert all(p._version == v + STEPS for p, v in zip(dut, versions))   # _bump_versions
    if not hp.get("weight_decay"):   # zero gradient and no decay: the parameter does not move, bit for bit
        assert torch.equal(dut[ZERO].detach().cpu().view(torch.int32), cpu[ZERO].view(torch.int32))
        assert not bool(state["square_avg"][ZERO].any())


# ---------------------------------------------------------------- state_dict ---
SMALL = ((5,), (4097,), (7, 9))


@pytest.mark.parametrize("momentum,centered", [(0.0, False), (0.9, False), (0.0, True), (0.9, True)])
def test_state_keys_equal_torchs(cuda, momentum, centered):
    cpu, grads = _inputs(SMALL, 9, 1)
    hp = dict(lr=1e-3, momentum=momentum, centered=centered)
    t32 = R.torch_fp32(cpu, grads, **hp)
    dut = [torch.nn.Parameter(t) for t in _to_dev(cpu, cuda)]
    opt = RMSprop(dut, **hp)
    for p, g in zip(dut, grads[0]):
        p.grad = g.to(cuda)
    opt.step()
    torch.cuda.synchronize()
    sd_t, sd_d = t32["optimizer"].state_dict(), opt.state_dict()
    assert sd_t["state"].keys() == sd_d["state"].keys()
    for i in sd_t["state"]:
        assert set(sd_t["state"][i]) == set(sd_d["state"][i]), (momentum, centered)
        assert float(sd_t["state"][i]["step"]) == float(sd_d["state"][i]["step"]) == 1.0
    assert set(sd_t["param_groups"][0]) | {"eps_in_sqrt", "lr_end", "anneal_steps"} == set(sd_d["param_groups"][0])


def test_torch_state_dict_loads_and_continues_and_loads_back(cuda):
    hp = CASES["centered + momentum"]
    cpu, grads = _inputs()
    head, tail = grads[:3], grads[3:]
    t3 = R.torch_fp32(cpu, head, **hp)                       # torch, fp32 on the CPU, three steps
    sd = copy.deepcopy(t3["optimizer"].state_dict())   # (torch is stepped on below: its step tensors are shared)
    start = [torch.from_numpy(p.astype(np.float32)) for p in t3["params"]]
    dut = [torch.nn.Parameter(t) for t in _to_dev(start, cuda)]
    opt = RMSprop(dut, **hp)
    opt.load_state_dict(sd)
    for p in dut:
        st = opt.state[p]
        assert float(st["step"]) == 3.0 and all(st[k].is_cuda for k in R.used(dict(R.DEFAULTS, **hp)))
    assert opt.param_groups[0]["eps_in_sqrt"] is False and opt.param_groups[0]["anneal_steps"] == 0
    for gs in tail:
        for p, g in zip(dut, gs):
            p.grad = g.to(cuda)
        opt.step()
    torch.cuda.synchronize()
    # the statement and torch itself, both continued from torch's state after three steps
    ref = R.run(t3["params"], tail, state=t3, applied=3, **hp)
    for gs in tail:
        for p, g in zip(t3["optimizer"].param_groups[0]["params"], gs):
            p.grad = g.clone()
        t3["optimizer"].step()
    o = t3["optimizer"]
    tp = o.param_groups[0]["params"]
    t6 = {"params": [p.detach().numpy() for p in tp]}
    for k in R.used(dict(R.DEFAULTS, **hp)):
        t6[k] = [o.state[p][k].numpy() for p in tp]
    state = {k: [opt.state[p][k] for p in dut] for k in R.used(dict(R.DEFAULTS, **hp))}
    _check_all(dut, state, ref, t6, hp, "continued from a torch state_dict")
    assert all(float(opt.state[p]["step"]) == 6.0 for p in dut)
    # and back: torch.optim.RMSprop takes the drop-in's state_dict
    back_p = [p.detach().cpu().clone().requires_grad_(True) for p in dut]
    back = torch.optim.RMSprop(back_p, foreach=False, **hp)
    back.load_state_dict(opt.state_dict())
    for p, q in zip(back_p, dut):
        assert float(back.state[p]["step"]) == 6.0
        for k in R.used(dict(R.DEFAULTS, **hp)):
            assert torch.equal(back.state[p][k], opt.state[q][k].cpu())
    for p, g in zip(back_p, tail[0]):
        p.grad = g.clone()
    back.step()   # torch steps on it
    assert all(float(back.state[p]["step"]) == 7.0 for p in back_p)


# --------------------------------------------------------------------- guard ---
def _raw_setup(cuda, hp, shapes=None, offset=(OFFSET,), seed=5):
    cpu, grads = _inputs(shapes, seed) if shapes is not None else _inputs()
    ps = _to_dev(cpu, cuda, offset)
    v, b, a = _state(ps, hp, offset)
    return cpu, grads, ps, v, b, a


def _all(ps, v, b, a):
    return ps + v + (b or []) + (a or [])


def test_guard(cuda):
    hp = dict(lr=1e-3, momentum=0.9, centered=True, lr_end=1e-4, anneal_steps=3)
    cpu, grads, ps, v, b, a = _raw_setup(cuda, hp)
    g0, g1 = _to_dev(grads[0], cuda), _to_dev(grads[1], cuda)
    step_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
    guard = torch.zeros(1, device=cuda)
    N.rmsprop_step(_hp(**hp), 0, ps, g0, v, b, a, guard=guard, step_dev=step_dev)
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 1 and not torch.equal(ps[0].cpu(), cpu[0])
    # a non-zero guard: parameters and state bit-identical, the counter where it was
    before = _bits(_all(ps, v, b, a))
    for value in (1.0, 3.0, -1.0, NAN):
        guard.fill_(value)
        N.rmsprop_step(_hp(**hp), 0, ps, g1, v, b, a, guard=guard, step_dev=step_dev)
        torch.cuda.synchronize()
        assert _same(before, _bits(_all(ps, v, b, a))) and int(step_dev.item()) == 1, value
    # a zero guard is the unguarded call, bit for bit
    outs = []
    for gd in (torch.zeros(1, device=cuda), None):
        q = _to_dev(cpu, cuda, (OFFSET,))
        qv, qb, qa = _state(q, hp, (OFFSET,))
        sd = torch.zeros(1, dtype=torch.int32, device=cuda)
        for gs in (g0, g1):
            N.rmsprop_step(_hp(**hp), 0, q, gs, qv, qb, qa, guard=gd, step_dev=sd)
        torch.cuda.synchronize()
        assert int(sd.item()) == 2
        outs.append(_bits(_all(q, qv, qb, qa)))
    assert _same(*outs)


# ---------------------------------------------------------------- non-finite ---
@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_nonfinite_step_is_skipped_and_not_counted(cuda, value):
    hp = CASES["impala"]
    cpu, grads, ps, v, b, a = _raw_setup(cuda, hp)
    bad = [g.clone() for g in grads[0]]
    bad[33].view(-1)[bad[33].numel() - 1] = value
    gs = _to_dev(bad, cuda)
    stats = torch.full((4,), NAN, device=cuda)
    N.grad_norm(1.0, gs, stats, _scratch(gs, cuda))
    step_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
    before = _bits(_all(ps, v, b, a))
    N.rmsprop_step(_hp(**hp), 0, ps, gs, v, b, a, step_dev=step_dev, clip=stats)      # device count
    N.rmsprop_step(_hp(**hp), 1, ps, gs, v, b, a, clip=stats)                         # host count, no guard
    torch.cuda.synchronize()
    assert float(stats[2]) == 1.0 and int(step_dev.item()) == 0
    assert _same(before, _bits(_all(ps, v, b, a)))
    # the next finite step applies, as update 1
    good = _to_dev(grads[0], cuda)
    N.grad_norm(INF, good, stats, _scratch(good, cuda))
    N.rmsprop_step(_hp(**hp), 0, ps, good, v, b, a, step_dev=step_dev, clip=stats)
    torch.cuda.synchronize()
    assert float(stats[2]) == 0.0 and int(step_dev.item()) == 1
    ref = R.run(cpu, [grads[0]], **hp)
    _check_all(ps, {"square_avg": v}, ref, None, hp, "after the skipped step")


# ---------------------------------------------------------------------- clip ---
def test_clip(cuda):
    hp = CASES["weight_decay"]
    cpu, grads = _inputs()
    g0, g1 = _to_dev(grads[0], cuda), _to_dev(grads[1], cuda)
    n0 = C.norm64(grads[0])
    # a coefficient of exactly 1 is stats = NULL, bit for bit
    outs = []
    for clip in (False, True):
        ps = _to_dev(cpu, cuda, (OFFSET,))
        v, b, a = _state(ps, hp, (OFFSET,))
        stats = torch.full((4,), NAN, device=cuda)
        if clip:
            N.grad_norm(2.0 * n0, g0, stats, _scratch(g0, cuda))
        N.rmsprop_step(_hp(**hp), 1, ps, g0, v, b, a, clip=stats if clip else None)
        torch.cuda.synchronize()
        if clip:
            assert float(stats[1]) == 1.0 and float(stats[2]) == 0.0
        outs.append(_bits(_all(ps, v, b, a)))
    assert _same(*outs)
    # a clipped step, then an unclipped one: the statement on fp32(g * coef)
    ps = _to_dev(cpu, cuda, (OFFSET,))
    v, b, a = _state(ps, hp, (OFFSET,))
    stats = torch.full((4,), NAN, device=cuda)
    step_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
    coefs = []
    for gs, limit in ((g0, 0.5 * n0), (g1, INF)):
        keep = [t.clone() for t in gs]
        N.grad_norm(limit, gs, stats, _scratch(gs, cuda))
        N.rmsprop_step(_hp(**hp), 0, ps, gs, v, b, a, step_dev=step_dev, clip=stats)
        torch.cuda.synchronize()
        coefs.append(np.float32(stats[1].item()))
        assert _same(keep, gs)   # the gradients themselves are not written
    assert 0.0 < coefs[0] < 1.0 and coefs[1] == 1.0 and int(step_dev.item()) == 2
    assert C.ulps(coefs[0], C.reference(grads[0], 0.5 * n0)["stats"][1]) <= 1
    ref = R.run(cpu, grads[:2], coef=coefs, **hp)
    t32 = R.torch_fp32(cpu, grads[:2], coef=coefs, **hp)
    _check_all(ps, {"square_avg": v}, ref, t32, hp, "clipped")


# ------------------------------------------------------------------ schedule ---
def test_schedule(cuda):
    hp = dict(lr=1e-2, lr_end=0.0, anneal_steps=4)
    cpu, grads, ps, v, b, a = _raw_setup(cuda, hp)
    step_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
    guard = torch.zeros(1, device=cuda)
    skip = [False, True, False, True, False, False]     # six calls, two of them guarded out
    for gs, s in zip(grads, skip):
        guard.fill_(1.0 if s else 0.0)
        N.rmsprop_step(_hp(**hp), 0, ps, _to_dev(gs, cuda), v, b, a, guard=guard, step_dev=step_dev)
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 4
    ref = R.run(cpu, grads, skip=skip, **hp)
    assert ref["lrs"] == [R.schedule(n, 1e-2, 0.0, 4) for n in range(4)]
    assert np.allclose(ref["lrs"], [1e-2, 7.5e-3, 5e-3, 2.5e-3], rtol=1e-15, atol=0.0)
    t32 = R.torch_fp32(cpu, grads, skip=skip, **hp)
    _check_all(ps, {"square_avg": v}, ref, t32, hp, "annealed")
    # the same applied updates at a constant lr are far outside the tolerance: the anneal is what was checked
    wrong = R.run(cpu, [g for g, s in zip(grads, skip) if not s], lr=1e-2)["params"][0]
    assert R.distance(ps[0], wrong) > 100 * TOL
    # n = 4 = anneal_steps, lr_end = 0: a further update leaves the parameters bit-identical; square_avg moves
    pb, vb = _bits(ps), _bits(v)
    guard.fill_(0.0)
    N.rmsprop_step(_hp(**hp), 0, ps, _to_dev(grads[0], cuda), v, b, a, guard=guard, step_dev=step_dev)
    torch.cuda.synchronize()
    assert _same(pb, _bits(ps)) and int(step_dev.item()) == 5
    moved = [not torch.equal(x, y) for x, y in zip(vb, _bits(v))]
    assert all(m for i, m in enumerate(moved) if i not in (ZERO, len(SHAPES) - 1)) and not moved[ZERO]


def test_host_count_equals_device_count(cuda):
    """step_dev = NULL with the host's step = 1, 2, ... is the device-counted run bit for bit when
    nothing is skipped: one statement of lr_t in double for both, past the end of the anneal too."""
    hp = dict(lr=7e-4, lr_end=1e-4, anneal_steps=3, momentum=0.9)
    cpu, grads = _inputs()
    outs = []
    for device_count in (True, False):
        ps = _to_dev(cpu, cuda, (OFFSET,))
        v, b, a = _state(ps, hp, (OFFSET,))
        step_dev = torch.zeros(1, dtype=torch.int32, device=cuda) if device_count else None
        for k, gs in enumerate(grads[:5]):
            N.rmsprop_step(_hp(**hp), k + 1, ps, _to_dev(gs, cuda), v, b, a, step_dev=step_dev)
        torch.cuda.synchronize()
        outs.append(_bits(_all(ps, v, b, a)))
    assert _same(*outs)
    ref = R.run(cpu, grads[:5], **hp)
    assert ref["lrs"][3] == ref["lrs"][4] == 1e-4
    _check_all(ps, {"square_avg": v, "momentum_buffer": b}, ref, R.torch_fp32(cpu, grads[:5], **hp), hp, "host count")


# ------------------------------------------------------- more than one table ---
MANY = tuple([(1 + (i * 37) % 300,) for i in range(48)] + [(0,), (R.CHUNK + 5,), (77,)])   # 51 tensors: 48 + 3


def test_more_than_48_tensors(cuda):
    hp = dict(lr=1e-3, lr_end=1e-4, anneal_steps=2, momentum=0.9, centered=True)
    cpu, grads = _inputs(MANY, 13, 2)
    outs = []
    for together in (True, False):
        ps = _to_dev(cpu, cuda)
        v, b, a = _state(ps, hp)
        step_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
        for k, gs in enumerate(grads):
            gd = _to_dev(gs, cuda)
            if together:
                N.rmsprop_step(_hp(**hp), 0, ps, gd, v, b, a, step_dev=step_dev)
            else:   # tensor by tensor, the host counting
                for i in range(len(ps)):
                    N.rmsprop_step(_hp(**hp), k + 1, [ps[i]], [gd[i]], [v[i]], [b[i]], [a[i]])
        torch.cuda.synchronize()
        if together:
            assert int(step_dev.item()) == 2   # once per step, not once per table
        outs.append(_bits(_all(ps, v, b, a)))
    assert _same(*outs)
    assert not torch.equal(ps[50].cpu(), cpu[50]) and not torch.equal(ps[0].cpu(), cpu[0])


def test_nothing_to_update_still_counts(cuda):
    step_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
    N.rmsprop_step(_hp(), 0, [], [], [], step_dev=step_dev)
    e = [torch.empty(0, device=cuda)]
    N.rmsprop_step(_hp(), 0, e, e, e, step_dev=step_dev)
    N.rmsprop_step(_hp(), 1, e, e, e)
    guard = torch.ones(1, device=cuda)
    N.rmsprop_step(_hp(), 0, [], [], [], step_dev=step_dev, guard=guard)
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 2


def test_unused_buffers_are_never_touched(cuda):
    """IMPALA's variant is given neither a momentum buffer nor grad_avg (NULL arrays); given
    NaN-filled ones all the same, it leaves them NaN and computes the same bits."""
    hp = CASES["impala"]
    cpu, grads = _inputs()
    g0 = _to_dev(grads[0], cuda)
    outs = []
    for given in (False, True):
        ps = _to_dev(cpu, cuda, (OFFSET,))
        v, _, _ = _state(ps, hp, (OFFSET,))
        junk = [torch.full_like(p, NAN) for p in ps] if given else None
        N.rmsprop_step(_hp(**hp), 1, ps, g0, v, junk, junk)
        torch.cuda.synchronize()
        if given:
            assert all(bool(torch.isnan(j).all()) for j in junk)
        outs.append(_bits(ps + v))
    assert _same(*outs)


# ------------------------------------------------------------------- learner ---
AG_A = 18
AG_HP = dict(gamma=0.97, lam=0.9, rho_bar=1.3, c_bar=0.8, pg_rho_bar=2.0, baseline_cost=0.5, entropy_cost=0.01)


def _agent_inputs(T, B):
    """The inputs of tests/test_gpu_vtrace.py's learner test, rebuilt here."""
    x = VR.make_inputs(T, B, AG_A, 23)
    x["done"][:] = 0
    x["done"][1, 0] = 1.0
    frames = torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3)).astype(np.float32))
    return frames, {k: x[k] for k in ("actions", "rewards", "behaviour_logp", "done", "bootstrap")}


def test_learner_rmsprop(cuda):
    from aaa_amd.learner import Learner
    T, B = 3, 2
    hp = dict(AG_HP, scale=1.0 / (T * B))
    frames, x = _agent_inputs(T, B)
    frames = frames.to(cuda).contiguous()
    d = {k: v.to(cuda) for k, v in x.items()}
    # the gradient norm of this iteration, from a learner that does not clip
    probe = Learner(B=B, T=T, device=cuda, optimizer="rmsprop")
    assert not hasattr(probe, "exp_avg") and not hasattr(probe, "exp_avg_sq")      # only the state it uses
    assert probe.momentum_buf is None and probe.grad_avg is None and probe.rmsprop == Learner.RMSPROP_DEFAULTS
    probe.step_vtrace(frames, **d, **hp)
    torch.cuda.synchronize()
    n0 = C.norm64([probe.grads.cpu()])
    assert math.isfinite(n0) and n0 > 0.0
    lr = Learner(B=B, T=T, device=cuda, optimizer="rmsprop", max_grad_norm=0.5 * n0, lr=6e-4, lr_anneal_steps=4,
                 lr_end=1e-4)
    assert lr.current_lr() == R.schedule(0, 6e-4, 1e-4, 4) and abs(lr.current_lr() - 6e-4) < 1e-18
    before = lr.flat.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("error")
    try:
        logits1, _, _ = lr.train_step_vtrace(frames, **d, **hp)      # no host read in the iteration
        logits1 = logits1.clone()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert not torch.equal(lr.flat, before) and bool(torch.isfinite(lr.flat).all())
    assert lr.opt_steps == 1
    assert lr.current_lr() == rmsprop_lr(1, 6e-4, 1e-4, 4) == R.schedule(1, 6e-4, 1e-4, 4)
    rep = lr.clip_report()
    assert 0.0 < rep["coef"] < 1.0 and rep["nonfinite"] == 0
    grads = lr.grads.cpu()
    ref = R.run([before.cpu()], [[grads]], coef=[np.float32(rep["coef"])], lr=6e-4, lr_end=1e-4, anneal_steps=4,
                **Learner.RMSPROP_DEFAULTS)
    _check_all([lr.flat], {"square_avg": [lr.square_avg]}, ref, None, Learner.RMSPROP_DEFAULTS, "learner")
    # the next forward runs on the updated weights: a fresh learner given them computes the same logits
    logits2, _, _ = lr.step_vtrace(frames, **d, **hp)
    fresh = Learner(B=B, T=T, device=cuda, optimizer="rmsprop")
    fresh.flat.copy_(lr.flat)
    logits3, _, _ = fresh.step_vtrace(frames, **d, **hp)
    torch.cuda.synchronize()
    assert torch.equal(logits2, logits3)
    print(f"logits moved by {rel_err(logits2.cpu().numpy(), logits1.cpu().numpy()):.3e} (norm-relative)")
    assert not torch.equal(logits2, logits1)
    lr.check_health()
    # a NaN gradient: skipped, not counted, the schedule where it was
    state = [t.clone() for t in (lr.flat, lr.square_avg)]
    bad = dict(d, actions=d["actions"].clone())
    bad["actions"][1, 0] = AG_A
    lr.train_step_vtrace(frames, **bad, **hp)
    torch.cuda.synchronize()
    assert _same(state, (lr.flat, lr.square_avg)) and lr.opt_steps == 1 and lr.clip_report()["nonfinite"] == 1
    assert lr.current_lr() == R.schedule(1, 6e-4, 1e-4, 4)
    lr.check_health()
    # momentum and centered learners allocate those buffers and use them
    mc = Learner(B=B, T=T, device=cuda, optimizer="rmsprop", rmsprop=dict(momentum=0.9, centered=True))
    mc.train_step_vtrace(frames, **d, **hp)
    torch.cuda.synchronize()
    assert mc.opt_steps == 1 and bool(mc.momentum_buf.any()) and bool(mc.grad_avg.any())
    mc.check_health()


def test_learner_adam_is_unchanged(cuda):
    """optimizer="adam" is the learner as it was: no RMSProp state, and one iteration applies the
    counted Adam's update bit for bit.  The small-batch backward accumulates its split-K weight
    gradients with floating-point atomics (csrc/epilogues.h), so two runs of one iteration can
    differ in the gradients' last bits whatever the optimizer does (tests/test_gpu_clip.py): the
    two learners' gradients are compared at 1e-6, and each learner's parameters and moments bit
    for bit with the counted Adam replayed on that learner's own gradients from the same start."""
    from aaa_amd.learner import Learner
    T, B = 3, 2
    hp = dict(AG_HP, scale=1.0 / (T * B))
    frames, x = _agent_inputs(T, B)
    frames = frames.to(cuda).contiguous()
    d = {k: v.to(cuda) for k, v in x.items()}
    default, adam = Learner(B=B, T=T, device=cuda), Learner(B=B, T=T, device=cuda, optimizer="adam")
    start = default.flat.clone()
    assert torch.equal(start, adam.flat)
    for ln in (default, adam):
        for name in ("square_avg", "momentum_buf", "grad_avg", "rmsprop"):
            assert not hasattr(ln, name), name
        assert ln.optimizer == "adam" and ln.current_lr() == ln.lr == 1e-3
        ln.train_step_vtrace(frames, **d, **hp)
    torch.cuda.synchronize()
    print(f"gradient elements that differ between the two learners: {int((default.grads != adam.grads).sum())}; "
          f"parameters equal: {torch.equal(default.flat, adam.flat)}")
    assert_close(adam.grads.cpu().numpy(), default.grads.cpu().numpy(), 1e-6, "grads with optimizer='adam'")
    for ln in (default, adam):
        p, m, v = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
        sd = torch.zeros(1, dtype=torch.int32, device=cuda)
        adam_flat_(p, ln.grads, m, v, 0, lr=ln.lr, guard=ln.guard, step_dev=sd)
        torch.cuda.synchronize()
        assert torch.equal(ln.flat, p) and torch.equal(ln.exp_avg, m) and torch.equal(ln.exp_avg_sq, v)
        assert ln.opt_steps == 1
        ln.check_health()
    with pytest.raises(ValueError, match="lr_anneal_steps"):
        Learner(B=B, T=T, device=cuda, optimizer="adam", lr_anneal_steps=5)
