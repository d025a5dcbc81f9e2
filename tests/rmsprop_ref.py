"""The float64 statement of the fused RMSProp update (include/aaa.h
``aaa_rmsprop_step``) and its learning-rate schedule, in numpy: torch's
``_single_tensor_rmsprop`` op order with both placements of eps, the guard /
non-finite skip (a skipped step moves neither the state nor the schedule) and
the clip coefficient (the gradient is the fp32 product ``grad * coef``, as the
kernel forms it, before anything else reads it).
tests/test_rmsprop_emulation.py checks it against ``torch.optim.RMSprop`` on
float64 parameters; the GPU tests (tests/test_gpu_rmsprop.py) compare the
kernel to it."""
from __future__ import annotations

import math

import numpy as np
import torch

CHUNK = 4096   # csrc/optim.hip kAdamChunk: elements per workgroup
DEFAULTS = dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, maximize=False,
                eps_in_sqrt=False, lr_end=0.0, anneal_steps=0)
STATE = ("square_avg", "momentum_buffer", "grad_avg")


def schedule(n: int, lr: float, lr_end: float = 0.0, anneal_steps: int = 0) -> float:
    """The learning rate of the update after ``n`` applied ones; anneal_steps = 0: constant."""
    if anneal_steps <= 0:
        return float(lr)
    return float(lr_end) + (float(lr) - float(lr_end)) * max(0.0, 1.0 - n / anneal_steps)


def _np64(t):
    return np.array(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)


def used(hp) -> tuple:
    """The state tensors a variant keeps, torch's names."""
    return ("square_avg",) + (("momentum_buffer",) if hp["momentum"] > 0 else ()) + (
        ("grad_avg",) if hp["centered"] else ())


def update(p, g, st, lr_t, hp):
    """One element-wise update in float64, in place: ``p`` and the arrays of ``st`` (used(hp))."""
    if hp["maximize"]:
        g = -g
    if hp["weight_decay"] != 0:
        g = g + hp["weight_decay"] * p
    v = st["square_avg"]
    v *= hp["alpha"]
    v += (1.0 - hp["alpha"]) * g * g
    s = v
    if hp["centered"]:
        a = st["grad_avg"]
        a += (1.0 - hp["alpha"]) * (g - a)
        s = v - a * a
    avg = np.sqrt(s + hp["eps"]) if hp["eps_in_sqrt"] else np.sqrt(s) + hp["eps"]
    if hp["momentum"] > 0:
        b = st["momentum_buffer"]
        b *= hp["momentum"]
        b += g / avg
        p -= lr_t * b
    else:
        p -= lr_t * (g / avg)


def scaled(g, coef):
    """``grad * coef`` as the kernel forms it: one fp32 multiply (coef None or 1: the gradient itself)."""
    g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
    if coef is None or np.float32(coef) == np.float32(1.0):
        return g
    return g.astype(np.float32) * np.float32(coef)


def run(params, steps, skip=None, coef=None, state=None, applied: int = 0, **hparams) -> dict:
    """``params``: fp32 (or fp64) tensors / arrays; ``steps``: per step, one gradient per
    parameter; ``skip``: per step, True when the guard or the non-finite flag refuses it;
    ``coef``: per step, the fp32 clip coefficient or None; ``state`` / ``applied``: where a
    run continues from.  Returns {"params", "square_avg", "momentum_buffer", "grad_avg":
    lists of float64 arrays (the unused ones None), "applied": updates applied, "lrs":
    the lr_t each applied update used}."""
    hp = dict(DEFAULTS, **hparams)
    ps = [_np64(p) for p in params]
    st = [{k: (np.zeros_like(p) if state is None else _np64(state[k][i])) for k in used(hp)}
          for i, p in enumerate(ps)]
    lrs = []
    for k, gs in enumerate(steps):
        if skip is not None and skip[k]:
            continue
        lr_t = schedule(applied, hp["lr"], hp["lr_end"], hp["anneal_steps"])
        c = None if coef is None else coef[k]
        for p, g, s in zip(ps, gs, st):
            update(p, _np64(scaled(g, c)), s, lr_t, hp)
        lrs.append(lr_t)
        applied += 1
    out = {"params": ps, "applied": applied, "lrs": lrs}
    for k in STATE:
        out[k] = [s[k] for s in st] if k in used(hp) else None
    return out


def torch_fp32(params, steps, skip=None, coef=None, **hparams) -> dict:
    """The same run by ``torch.optim.RMSprop(foreach=False)`` in fp32 on the CPU, the schedule
    written into the group's lr before each applied step (torch has no eps_in_sqrt: refused).
    Its distance from run() is what fp32 in torch's op order costs on these inputs."""
    hp = dict(DEFAULTS, **hparams)
    assert not hp["eps_in_sqrt"], "torch.optim.RMSprop has no eps inside the square root"
    ps = [torch.as_tensor(np.asarray(p), dtype=torch.float32).clone().requires_grad_(True) for p in params]
    opt = torch.optim.RMSprop(ps, lr=hp["lr"], alpha=hp["alpha"], eps=hp["eps"], weight_decay=hp["weight_decay"],
                              momentum=hp["momentum"], centered=hp["centered"], maximize=hp["maximize"], foreach=False)
    applied = 0
    for k, gs in enumerate(steps):
        if skip is not None and skip[k]:
            continue
        opt.param_groups[0]["lr"] = schedule(applied, hp["lr"], hp["lr_end"], hp["anneal_steps"])
        c = None if coef is None else coef[k]
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(np.array(scaled(g, c), dtype=np.float32))
        opt.step()
        applied += 1
    out = {"params": [p.detach().numpy().astype(np.float64) for p in ps], "applied": applied, "optimizer": opt}
    for k in STATE:
        out[k] = ([opt.state[p][k].numpy().astype(np.float64) if opt.state[p] else np.zeros(p.shape) for p in ps]
                  if k in used(hp) else None)
    return out


def distance(got, ref) -> float:
    """max |got - ref| over max |ref| of one tensor (0 for an empty one)."""
    got, ref = _np64(got), _np64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return math.inf
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))
