"""Device V-trace actor-critic loss (csrc/loss.hip, aaa_vtrace) against its
float64 statement (tests/vtrace_ref.py, itself checked on the CPU by
tests/test_vtrace_emulation.py) on the same fp32 inputs, its structural
properties bit for bit, the autograd surface, the loss driving the
hand-written BPTT through the agent, and the learner iteration built on it.

Tolerances are the sibling kernel's (tests/test_gpu_reinforce.py): cotangents
and targets to 1e-5 of the reference tensor's largest magnitude, each loss
part to 1e-4 max(1, |ref|)."""
import functools
import warnings

import numpy as np
import pytest
import torch

from helpers import assert_close, detinit
from oracle import ref_cpu

import attention
import vtrace_ref as R
from aaa_amd.vtrace import vtrace_cotangents, vtrace_loss

pytestmark = pytest.mark.gpu
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and fp64 reference of case i, computed once and shared (read-only)."""
    x = R.case_inputs(i)
    return x, R.reference(**x, **R.case_hparams(R.CASES[i]))


def _dev(x, dev):
    return {k: (v.to(dev) if v is not None else None) for k, v in x.items()}


def _run(x, dev, extras=True, **hp):
    """aaa_vtrace on the inputs ``x`` (CPU tensors) into NaN-filled outputs -> CPU tensors."""
    d = _dev(x, dev)
    T, B, A = x["logits"].shape
    out = dict(dlogits=torch.full((T, B, A), NAN, device=dev), dvalues=torch.full((T, B, A), NAN, device=dev))
    if extras:
        out.update(vs=torch.full((T, B), NAN, device=dev), pg_adv=torch.full((T, B), NAN, device=dev),
                   parts=torch.full((B, 3), NAN, device=dev))
    vtrace_cotangents(d["logits"], d["values"], d["actions"], d["rewards"], d["behaviour_logp"], d["done"],
                      d["bootstrap"], out["dlogits"], out["dvalues"], out.get("vs"), out.get("pg_adv"),
                      out.get("parts"), **hp)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check(out, ref, what=""):
    for k in ("dlogits", "dvalues", "vs", "pg_adv"):
        if k not in out:
            continue
        assert bool(torch.isfinite(out[k]).all()), f"{what}{k}: an element was not written (or is not finite)"
        err = float((out[k].double() - ref[k]).abs().max())
        bound = 1e-5 * float(ref[k].abs().max())
        print(f"{what}{k}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (what, k, err, bound)
    if "parts" in out:
        for j, name in enumerate(("pg", "baseline", "entropy")):
            for b in range(ref["parts"].shape[0]):
                r = float(ref["parts"][b, j])
                assert abs(float(out["parts"][b, j]) - r) <= 1e-4 * max(1.0, abs(r)), (what, name, b)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_kernel_matches_fp64_reference(cuda, i):
    c = R.CASES[i]
    x, ref = _case(i)
    out = _run(x, cuda, **R.case_hparams(c))
    _check(out, ref)
    off = torch.ones(c["A"], dtype=torch.bool)
    off[c["vc"]] = False
    assert bool((out["dvalues"][..., off] == 0).all())   # written, and exactly zero
    # the optional outputs are optional
    bare = _run(x, cuda, extras=False, **R.case_hparams(c))
    assert torch.equal(bare["dlogits"], out["dlogits"]) and torch.equal(bare["dvalues"], out["dvalues"])


def test_row_permutation_permutes_every_output_bitwise(cuda):
    i = 2   # (20, 32, 18): eight workgroups of four rows
    x, _ = _case(i)
    hp = R.case_hparams(R.CASES[i])
    perm = torch.randperm(R.CASES[i]["B"], generator=torch.Generator().manual_seed(3))
    y = {k: (v[perm] if k == "bootstrap" else v[:, perm].contiguous()) if v is not None else None
         for k, v in x.items()}
    a, b = _run(x, cuda, **hp), _run(y, cuda, **hp)
    for k in ("dlogits", "dvalues", "vs", "pg_adv"):
        assert torch.equal(a[k][:, perm], b[k]), k
    assert torch.equal(a["parts"][perm], b["parts"])


@pytest.mark.parametrize("T,t0", [(20, 7), (65, 63), (140, 64)])
def test_done_isolates_the_steps_before_it_bitwise(cuda, T, t0):
    """done[t0, b] = 1: nothing of row b after t0 reaches its outputs at steps
    <= t0 (also across the 64-step chunks of the scan); the other rows do not move."""
    B, A, b = 3, 18, 1
    x = R.make_inputs(T, B, A, 41, done=False)
    x["done"] = torch.zeros(T, B)
    x["done"][t0, b] = 1.0
    y = {k: (v.clone() if v is not None else None) for k, v in x.items()}
    g = torch.Generator().manual_seed(5)
    y["logits"][t0 + 1:, b] = torch.randn(T - t0 - 1, A, generator=g) * 3
    y["values"][t0 + 1:, b] = torch.randn(T - t0 - 1, A, generator=g)
    y["rewards"][t0 + 1:, b] = torch.randn(T - t0 - 1, generator=g)
    y["bootstrap"][b] = 7.0
    hp = dict(lam=0.9, rho_bar=1.3, c_bar=0.8)
    p, q = _run(x, cuda, **hp), _run(y, cuda, **hp)
    for k in ("dlogits", "dvalues", "vs", "pg_adv"):
        assert torch.equal(p[k][:t0 + 1, b], q[k][:t0 + 1, b]), k
        assert not torch.equal(p[k][t0 + 1:, b], q[k][t0 + 1:, b]), k
        for o in (0, 2):
            assert torch.equal(p[k][:, o], q[k][:, o]), (k, o)
    _check(q, R.reference(**y, **hp), "changed tail: ")


def test_plain_bootstrapped_policy_gradient(cuda):
    """No entropy or baseline cost, on-policy, lambda = 1: the cotangents are the
    plain policy gradient's on the bootstrapped n-step advantage, and no value gradient."""
    T, B, A, gamma = 33, 5, 6, 0.95
    x = R.make_inputs(T, B, A, 17, mu=False, done=False)
    hp = dict(gamma=gamma, lam=1.0, entropy_cost=0.0, baseline_cost=0.0, scale=0.5)
    out = _run(x, cuda, **hp)
    _check(out, R.reference(**x, **hp))
    assert bool((out["dvalues"] == 0).all())
    ret, G = [None] * T, x["bootstrap"].double()
    for t in range(T - 1, -1, -1):
        G = x["rewards"][t].double() + gamma * G
        ret[t] = G
    adv = torch.stack(ret) - x["values"][..., 0].double()
    onehot = torch.nn.functional.one_hot(x["actions"].long(), A).double()
    pg = -0.5 * adv.unsqueeze(-1) * (onehot - torch.softmax(x["logits"].double(), -1))
    assert float((out["dlogits"].double() - pg).abs().max()) <= 1e-5 * float(pg.abs().max())


def test_out_of_range_action_poisons_its_row_only(cuda):
    """The kernel guards the action index: an action outside [0, A) reads nothing
    outside its row's A floats, that row's outputs are NaN, the other rows' are untouched."""
    i = 5   # (65, 3, 18): the bad actions sit in different 64-step chunks than most of the row
    x, _ = _case(i)
    hp = R.case_hparams(R.CASES[i])
    y = dict(x, actions=x["actions"].clone())
    y["actions"][64, 0] = 18
    y["actions"][3, 2] = -1
    y["actions"][40, 2] = 2 ** 31 - 1
    a, b = _run(x, cuda, **hp), _run(y, cuda, **hp)
    for k in ("dlogits", "dvalues", "vs", "pg_adv"):
        assert torch.equal(a[k][:, 1], b[k][:, 1]), k
        assert bool(torch.isnan(b[k][:, 0]).all()) and bool(torch.isnan(b[k][:, 2]).all()), k
    assert torch.equal(a["parts"][1], b["parts"][1]) and bool(torch.isnan(b["parts"][[0, 2]]).all())


# ------------------------------------------------------------- autograd ---
def test_backward_puts_the_cotangents_on_the_leaves(cuda):
    i = 9   # (50, 7, 6), non-default clips, costs and scale
    c = R.CASES[i]
    x, ref = _case(i)
    hp = R.case_hparams(c)
    d = _dev(x, cuda)
    lg, vl = d["logits"].requires_grad_(True), d["values"].requires_grad_(True)
    loss, vs, adv, parts = vtrace_loss(lg, vl, x["actions"], x["rewards"], x["behaviour_logp"], x["done"],
                                       x["bootstrap"], return_extras=True, **hp)
    (2.5 * loss).backward()
    torch.cuda.synchronize()
    raw = _run(x, cuda, **hp)
    assert torch.equal(lg.grad.cpu(), raw["dlogits"] * 2.5) and torch.equal(vl.grad.cpu(), raw["dvalues"] * 2.5)
    assert torch.equal(vs.cpu(), raw["vs"]) and torch.equal(adv.cpu(), raw["pg_adv"])
    assert torch.equal(parts.cpu(), raw["parts"])
    assert not (vs.requires_grad or adv.requires_grad or parts.requires_grad)
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"])))


def test_bootstrap_last_is_the_explicit_call_on_t_minus_one_steps(cuda):
    i = 4   # (64, 3, 18), value_col = A - 1
    c = R.CASES[i]
    x, _ = _case(i)
    hp = R.case_hparams(c)
    T = c["T"]
    d = _dev(x, cuda)
    lg, vl = d["logits"].requires_grad_(True), d["values"].requires_grad_(True)
    loss = vtrace_loss(lg, vl, x["actions"], x["rewards"], x["behaviour_logp"], x["done"], "last", **hp)
    loss.backward()
    lg2, vl2 = (t.detach()[:T - 1].clone().requires_grad_(True) for t in (lg, vl))
    loss2 = vtrace_loss(lg2, vl2, x["actions"][:T - 1], x["rewards"][:T - 1], x["behaviour_logp"][:T - 1],
                        x["done"][:T - 1], x["values"][T - 1, :, c["vc"]], **hp)
    loss2.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2)
    assert torch.equal(lg.grad[:T - 1], lg2.grad) and torch.equal(vl.grad[:T - 1], vl2.grad)
    assert bool((lg.grad[T - 1] == 0).all()) and bool((vl.grad[T - 1] == 0).all())
    # the (T, B) inputs may also come already cut to T - 1 steps
    lg3, vl3 = (t.detach().clone().requires_grad_(True) for t in (lg, vl))
    vtrace_loss(lg3, vl3, x["actions"][:T - 1], x["rewards"][:T - 1], x["behaviour_logp"][:T - 1],
                x["done"][:T - 1], "last", **hp).backward()
    assert torch.equal(lg3.grad, lg.grad) and torch.equal(vl3.grad, vl.grad)


def test_surface_validates_before_any_launch(cuda):
    x, _ = _case(1)
    d = _dev(x, cuda)
    lg, vl = d["logits"].requires_grad_(True), d["values"].requires_grad_(True)
    for bad in (5, -1):
        a = x["actions"].clone()
        a[1, 1] = bad
        with pytest.raises(ValueError, match="actions must lie"):
            vtrace_loss(lg, vl, a, x["rewards"])
    with pytest.raises(ValueError):
        vtrace_loss(lg, vl[:, :, :4], x["actions"], x["rewards"])
    with pytest.raises(ValueError):
        vtrace_loss(lg, vl, x["actions"][:2], x["rewards"])
    with pytest.raises(ValueError):
        vtrace_loss(lg, vl, x["actions"], x["rewards"], value_col=5)
    with pytest.raises(RuntimeError, match="fp32"):
        vtrace_loss(lg.double(), vl.double(), x["actions"], x["rewards"])
    with pytest.raises(RuntimeError, match="gamma"):   # the C ABI's own refusal, surfaced
        vtrace_loss(lg, vl, x["actions"], x["rewards"], gamma=1.5)
    assert lg.grad is None and vl.grad is None


# ---------------------------------------------------- through the agent ---
AG_T, AG_B, AG_A = 4, 2, 18
AG_HP = dict(gamma=0.97, lam=0.9, rho_bar=1.3, c_bar=0.8, pg_rho_bar=2.0, baseline_cost=0.5, entropy_cost=0.01,
             scale=1.0 / (AG_T * AG_B))


def _agent_inputs(T=AG_T, B=AG_B):
    x = R.make_inputs(T, B, AG_A, 23)
    x["done"][:] = 0
    x["done"][1, 0] = 1.0
    frames = torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3)).astype(np.float32))
    return frames, {k: x[k] for k in ("actions", "rewards", "behaviour_logp", "done", "bootstrap")}


def _param_grads(ag):
    return {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().clone()
            for n, p in ag.named_parameters()}


def test_loss_drives_the_bptt_through_the_agent(cuda):
    frames, x = _agent_inputs()
    ag = attention.Agent(AG_A, grid=(11, 11))
    detinit.load_into(ag, detinit.deterministic_params(0, AG_A))
    ag.to(cuda)
    X = frames.to(cuda)
    ag.reset()
    lg, vl, _ = ag.unroll(X)
    vtrace_loss(lg, vl, **x, **AG_HP).backward()
    torch.cuda.synchronize()
    Ga = _param_grads(ag)
    # the same cotangents, taken from aaa_vtrace on the detached outputs, fed as a linear loss
    raw = _run(dict(x, logits=lg.detach().cpu(), values=vl.detach().cpu()), cuda, extras=False, **AG_HP)
    for p in ag.parameters():
        p.grad = None
    ag.reset()
    lg2, vl2, _ = ag.unroll(X)
    ((lg2 * raw["dlogits"].to(cuda)).sum() + (vl2 * raw["dvalues"].to(cuda)).sum()).backward()
    torch.cuda.synchronize()
    Gb = _param_grads(ag)
    for n in Ga:
        if float(Gb[n].abs().max()) == 0.0:
            assert float(Ga[n].abs().max()) == 0.0, n
        else:
            assert_close(Ga[n].numpy(), Gb[n].numpy(), 1e-6, "Ga vs Gb " + n)
    for n in ("policy_head.0.weight", "policy_head.0.bias", "values_head.0.weight", "values_head.0.bias"):
        assert float(Ga[n].abs().max()) > 0.0, n
    # the CPU oracle's unroll with the fp64 statement of the loss on top, at the fp32 gate
    P = ref_cpu.tensor_params(detinit.deterministic_params(0, AG_A))
    rl, rv, _ = ref_cpu.unroll(P, frames)
    assert_close(lg.detach().cpu().numpy(), rl.detach().numpy(), 1e-4, "logits")
    assert_close(vl.detach().cpu().numpy(), rv.detach().numpy(), 1e-4, "values")
    R.loss_fp64(rl, rv, **x, **AG_HP)[0].backward()
    for n, p in P.items():
        if p.grad is None or float(p.grad.norm()) == 0.0:
            assert float(Ga[n].abs().max()) == 0.0, f"{n}: reference grad is exactly zero (Q1)"
        else:
            assert_close(Ga[n].numpy(), p.grad.numpy(), 1e-4, "grad " + n)


# -------------------------------------------------------------- learner ---
def _no_host_read(fn):
    """The host-read names a function's code (nested functions included) touches."""
    banned = {"item", "cpu", "tolist", "numpy", "synchronize", "nonzero"}
    code = fn.__code__ if hasattr(fn, "__code__") else fn
    hits = banned & set(code.co_names)
    for c in code.co_consts:
        if hasattr(c, "co_names"):
            hits |= _no_host_read(c)
    return hits


def test_learner_step_vtrace(cuda):
    from aaa_amd.learner import Learner
    T, B = 3, 2
    frames, x = _agent_inputs(T, B)
    frames = frames.to(cuda).contiguous()
    d = _dev(x, cuda)
    lr = Learner(B=B, T=T, device=cuda)
    lg, vl, parts = lr.step_vtrace(frames, **d, **AG_HP)
    torch.cuda.synchronize()
    g1 = lr.grads.clone()
    raw = _run(dict(x, logits=lg.cpu(), values=vl.cpu()), cuda, **AG_HP)
    assert torch.equal(parts.cpu(), raw["parts"])
    lg2, vl2 = lr.step(frames, raw["dlogits"].to(cuda), raw["dvalues"].to(cuda))
    torch.cuda.synchronize()
    assert torch.equal(lg, lg2) and torch.equal(vl, vl2)
    assert float(g1.abs().max()) > 0.0
    assert_close(g1.cpu().numpy(), lr.grads.cpu().numpy(), 1e-6, "step_vtrace vs step grads")
    lr.check_health()
    # a complete iteration: one Adam update, applied -- and nothing in it reads the device
    # from the host: torch raises on any synchronising call inside the block, and the
    # iteration's own code names no host read
    before, n0 = lr.flat.clone(), lr.opt_steps
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # "a prototype feature": it does catch .item() / .cpu() / nonzero()
        torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):   # the check is live: a host read does raise here
            lr.step_dev.item()
        lr.train_step_vtrace(frames, **d, **AG_HP)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert lr.opt_steps == n0 + 1
    assert not torch.equal(lr.flat, before) and bool(torch.isfinite(lr.flat).all())
    for fn in (Learner.train_step_vtrace, Learner.step_vtrace, Learner._forward, Learner._backward,
               Learner.optimizer_step, vtrace_cotangents):
        assert not _no_host_read(fn), (fn.__qualname__, _no_host_read(fn))
    # bootstrap="last": the last step's rows of the learner's cotangent buffers are zero
    lr.step_vtrace(frames, d["actions"], d["rewards"], d["behaviour_logp"], d["done"], "last", **AG_HP)
    torch.cuda.synchronize()
    dl, dv = lr._vt
    assert bool((dl[T - 1] == 0).all()) and bool((dv[T - 1] == 0).all()) and float(dl[:T - 1].abs().max()) > 0.0
    lr.check_health()
