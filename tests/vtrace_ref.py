"""The V-trace actor-critic loss (include/aaa.h aaa_vtrace) stated twice in
float64, for the tests of the device kernel (not a test module).

``reference``: torch fp64, batched; the loss is built with ``.detach()`` on vs
and the advantages and the cotangents come from ``autograd.grad``.
``literal``: a per-row, per-step Python loop over floats, with the cotangents
from the closed-form formulas.  tests/test_vtrace_emulation.py holds the two
against each other; tests/test_gpu_vtrace.py holds the kernel against the
first.  ``make_inputs`` / ``CASES`` are the inputs both use.
"""
from __future__ import annotations

import math

import torch

DEFAULTS = dict(gamma=0.99, lam=1.0, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, baseline_cost=0.5,
                entropy_cost=0.01, scale=1.0, value_col=0)

OFF_DEFAULT = dict(gamma=0.97, rho_bar=1.3, c_bar=0.8, pg_rho_bar=2.0, baseline_cost=0.25, entropy_cost=0.02,
                   scale=1.0 / 64)

# (T, B, A) of the issue, each with the optional inputs on and off somewhere; lam in {1, 0.9}; value_col
# in {0, A-1}; "hp" = the non-default clips / costs / scale.  The seed is the case's index.
CASES = [
    dict(T=1, B=1, A=2, mu=True, done=False, boot=True, lam=1.0, vc=0, hp={}),
    dict(T=3, B=2, A=5, mu=True, done=True, boot=False, lam=0.9, vc=4, hp=OFF_DEFAULT),
    dict(T=20, B=32, A=18, mu=True, done=True, boot=True, lam=1.0, vc=0, hp={}),
    dict(T=20, B=32, A=18, mu=False, done=False, boot=False, lam=0.9, vc=17, hp={}),
    dict(T=64, B=3, A=18, mu=True, done=True, boot=True, lam=0.9, vc=17, hp={}),
    dict(T=65, B=3, A=18, mu=True, done=True, boot=True, lam=1.0, vc=0, hp={}),
    dict(T=65, B=3, A=18, mu=True, done=False, boot=True, lam=0.9, vc=0, hp=OFF_DEFAULT),
    dict(T=517, B=1, A=18, mu=True, done=True, boot=True, lam=1.0, vc=0, hp={}),
    dict(T=517, B=1, A=18, mu=False, done=False, boot=True, lam=1.0, vc=17, hp={}),
    dict(T=50, B=7, A=6, mu=True, done=True, boot=True, lam=0.9, vc=5, hp=OFF_DEFAULT),
]


def case_id(c) -> str:
    return (f"T{c['T']}-B{c['B']}-A{c['A']}-{'mu' if c['mu'] else 'onp'}-{'done' if c['done'] else 'nodone'}-"
            f"{'boot' if c['boot'] else 'noboot'}-lam{c['lam']}-vc{c['vc']}{'-hp' if c['hp'] else ''}")


def case_hparams(c) -> dict:
    return dict(DEFAULTS, lam=c["lam"], value_col=c["vc"], **c["hp"])


def make_inputs(T, B, A, seed, mu=True, done=True, boot=True) -> dict:
    """fp32 inputs: logits ~ 3 N(0,1), values ~ N(0,1), uniform actions, sparse
    rewards (10 with probability 0.2, as tests/test_gpu_reinforce.py), the
    behaviour log-probs from independent logits ~ 3 N(0,1), done ~ Bernoulli(0.1)."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = dict(logits=torch.randn(T, B, A, generator=g) * 3, values=torch.randn(T, B, A, generator=g),
             actions=torch.randint(0, A, (T, B), generator=g, dtype=torch.int32),
             rewards=(torch.rand(T, B, generator=g) < 0.2).float() * 10)
    mu_logits = torch.randn(T, B, A, generator=g) * 3
    d = (torch.rand(T, B, generator=g) < 0.1).float()
    bs = torch.randn(B, generator=g)
    x["behaviour_logp"] = (torch.log_softmax(mu_logits.double(), -1)
                           .gather(-1, x["actions"].long().unsqueeze(-1)).squeeze(-1).float()) if mu else None
    x["done"] = d if done else None
    x["bootstrap"] = bs if boot else None
    return x


def case_inputs(i: int) -> dict:
    c = CASES[i]
    return make_inputs(c["T"], c["B"], c["A"], i, c["mu"], c["done"], c["boot"])


def ratios(x) -> torch.Tensor:
    """e^{log rho} (T, B) in fp64 (ones without behaviour log-probs)."""
    lpa = torch.log_softmax(x["logits"].double(), -1).gather(-1, x["actions"].long().unsqueeze(-1)).squeeze(-1)
    if x["behaviour_logp"] is None:
        return torch.ones_like(lpa)
    return (lpa - x["behaviour_logp"].double()).exp()


def loss_fp64(logits, values, actions, rewards, behaviour_logp=None, done=None, bootstrap=None, **hparams):
    """The loss in fp64 as a differentiable function of ``logits`` and
    ``values`` (vs, the advantages and the ratios detached): (loss, parts (B, 3),
    vs, pg_adv).  The inputs keep their autograd graph."""
    hp = dict(DEFAULTS, **hparams)
    vc = hp["value_col"]
    l, v = logits.double(), values.double()
    T, B, A = l.shape
    a = torch.as_tensor(actions).long().reshape(T, B)
    r = torch.as_tensor(rewards).double().reshape(T, B)
    logpi = torch.log_softmax(l, -1)
    p = logpi.exp()
    H = -(p * logpi).sum(-1)
    lpa = logpi.gather(-1, a.unsqueeze(-1)).squeeze(-1)
    V = v[..., vc]
    with torch.no_grad():
        ratio = (lpa - behaviour_logp.double().reshape(T, B)).exp() if behaviour_logp is not None else torch.ones_like(lpa)
        rho = ratio.clamp(max=hp["rho_bar"])
        c = hp["lam"] * ratio.clamp(max=hp["c_bar"])
        rho_pg = ratio.clamp(max=hp["pg_rho_bar"])
        g = hp["gamma"] * (1.0 - (done.reshape(T, B) != 0).double()) if done is not None else torch.full_like(r, hp["gamma"])
        VT = bootstrap.double().reshape(B) if bootstrap is not None else torch.zeros(B, dtype=torch.float64)
        Vn = torch.cat([V[1:], VT[None]])
        delta = rho * (r + g * Vn - V)
        xs, x = [None] * T, torch.zeros(B, dtype=torch.float64)
        for t in range(T - 1, -1, -1):
            x = delta[t] + g[t] * c[t] * x
            xs[t] = x
        vs = V + torch.stack(xs)
        adv = rho_pg * (r + g * torch.cat([vs[1:], VT[None]]) - V)
    parts = torch.stack([(-adv.detach() * lpa).sum(0), (0.5 * (vs.detach() - V) ** 2).sum(0), H.sum(0)], dim=1)
    loss = hp["scale"] * (parts[:, 0] + hp["baseline_cost"] * parts[:, 1] - hp["entropy_cost"] * parts[:, 2]).sum()
    return loss, parts, vs, adv


def reference(logits, values, actions, rewards, behaviour_logp=None, done=None, bootstrap=None, **hparams) -> dict:
    """fp64 outputs of aaa_vtrace for fp32 (or fp64) inputs: dlogits, dvalues
    (T, B, A), vs, pg_adv (T, B), parts (B, 3) and the scalar loss."""
    l = logits.detach().double().requires_grad_(True)
    v = values.detach().double().requires_grad_(True)
    loss, parts, vs, adv = loss_fp64(l, v, actions, rewards, behaviour_logp, done, bootstrap, **hparams)
    dl, dv = torch.autograd.grad(loss, (l, v))
    return dict(dlogits=dl, dvalues=dv, vs=vs, pg_adv=adv, parts=parts.detach(), loss=loss.detach())


def literal(logits, values, actions, rewards, behaviour_logp=None, done=None, bootstrap=None, **hparams) -> dict:
    """The same quantities from a literal loop over rows and steps on Python
    floats, the cotangents from the closed forms of include/aaa.h."""
    hp = dict(DEFAULTS, **hparams)
    vc, gamma, lam, scale = hp["value_col"], hp["gamma"], hp["lam"], hp["scale"]
    T, B, A = logits.shape
    L, Vv = logits.double().tolist(), values.double().tolist()
    act, rew = actions.reshape(T, B).tolist(), rewards.double().reshape(T, B).tolist()
    mu = behaviour_logp.double().reshape(T, B).tolist() if behaviour_logp is not None else None
    dn = done.reshape(T, B).tolist() if done is not None else None
    bs = bootstrap.double().reshape(B).tolist() if bootstrap is not None else None
    dl = torch.zeros(T, B, A, dtype=torch.float64)
    dv = torch.zeros(T, B, A, dtype=torch.float64)
    vs_o = torch.zeros(T, B, dtype=torch.float64)
    adv_o = torch.zeros(T, B, dtype=torch.float64)
    parts = torch.zeros(B, 3, dtype=torch.float64)
    for b in range(B):
        VT = bs[b] if bs is not None else 0.0
        x_next, vs_next, V_next = 0.0, VT, VT
        for t in range(T - 1, -1, -1):
            row = L[t][b]
            mx = max(row)
            lse = mx + math.log(sum(math.exp(v - mx) for v in row))
            logpi = [v - lse for v in row]
            p = [math.exp(v) for v in logpi]
            H = -sum(pk * lk for pk, lk in zip(p, logpi))
            a = act[t][b]
            V = Vv[t][b][vc]
            ratio = math.exp(logpi[a] - mu[t][b]) if mu is not None else 1.0
            rho, c, rho_pg = min(hp["rho_bar"], ratio), lam * min(hp["c_bar"], ratio), min(hp["pg_rho_bar"], ratio)
            g = gamma * (0.0 if dn is not None and dn[t][b] != 0 else 1.0)
            delta = rho * (rew[t][b] + g * V_next - V)
            x = delta + g * c * x_next
            vs = V + x
            adv = rho_pg * (rew[t][b] + g * vs_next - V)
            for k in range(A):
                dl[t, b, k] = scale * (-adv * ((1.0 if k == a else 0.0) - p[k]) + hp["entropy_cost"] * p[k] * (logpi[k] + H))
            dv[t, b, vc] = -scale * hp["baseline_cost"] * (vs - V)
            vs_o[t, b], adv_o[t, b] = vs, adv
            parts[b, 0] += -adv * logpi[a]
            parts[b, 1] += 0.5 * (vs - V) ** 2
            parts[b, 2] += H
            x_next, vs_next, V_next = x, vs, V
    loss = scale * (parts[:, 0] + hp["baseline_cost"] * parts[:, 1] - hp["entropy_cost"] * parts[:, 2]).sum()
    return dict(dlogits=dl, dvalues=dv, vs=vs_o, pg_adv=adv_o, parts=parts, loss=loss)
