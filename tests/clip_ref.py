"""The float64 statement of gradient clipping by global norm (include/aaa.h
``aaa_grad_norm`` / ``aaa_adam_step_clipped``), in numpy: the norm, the
coefficient with its IEEE cases, the non-finite flag, and the clipped Adam
step -- the fp32 multiply ``grad * coef`` followed by CPU
``torch.optim.Adam(foreach=False)``.  tests/test_clip_emulation.py checks it
against ``torch.nn.utils.clip_grad_norm_`` on float64 tensors; the GPU tests
(tests/test_gpu_clip.py) compare the kernels to it."""
from __future__ import annotations

import math

import numpy as np
import torch

CHUNK = 4096   # csrc/optim.hip kAdamChunk: elements per workgroup
EPS = 1e-6     # torch.nn.utils.clip_grad_norm_'s


def _flat64(grads):
    parts = [np.asarray(g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else g, dtype=np.float64).reshape(-1)
             for g in grads]
    return np.concatenate(parts) if parts else np.zeros(0)


def norm64(grads) -> float:
    """sqrt of the sum of the squares of every element, in float64 (exactly
    rounded sum for finite inputs; inf / NaN as IEEE gives them)."""
    a = _flat64(grads)
    sq = a * a
    if not np.all(np.isfinite(sq)):
        with np.errstate(invalid="ignore"):
            return float(np.sqrt(np.sum(sq)))
    return math.sqrt(_fsum_blocks(sq))


def _fsum_blocks(sq: np.ndarray) -> float:
    """math.fsum over block sums that are themselves math.fsum: within 2 ulp (double) of exact."""
    return math.fsum(math.fsum(sq[i:i + (1 << 16)].tolist()) for i in range(0, sq.size, 1 << 16))


def coefficient(norm: float, max_norm: float) -> float:
    """clamp(max_norm / (norm + 1e-6), max=1.0) in double: NaN norm -> NaN, inf norm -> 0
    (NaN when max_norm is inf too), max_norm = inf and a finite norm -> 1."""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = float(np.float64(max_norm) / (np.float64(norm) + np.float64(EPS)))
    return c if math.isnan(c) else min(1.0, c)


def reference(grads, max_norm: float, norm: float | None = None) -> dict:
    """{"norm", "coef" (float64), "nonfinite", "stats" (the 4 fp32 values the device writes)};
    ``norm``: norm64(grads) when the caller already has it."""
    n = norm64(grads) if norm is None else norm
    c = coefficient(n, max_norm)
    flag = 0.0 if math.isfinite(n) else 1.0
    with np.errstate(over="ignore"):
        stats = np.array([n, c, flag, max_norm], dtype=np.float64).astype(np.float32)
    return {"norm": n, "coef": c, "nonfinite": int(flag), "stats": stats}


def ulps(a, b) -> int:
    """Distance in fp32 units in the last place between two finite fp32 values."""
    def key(x):
        i = int(np.float32(x).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def same_f32(a, b) -> bool:
    """Equal as fp32 values, NaN equal to NaN."""
    a, b = np.float32(a), np.float32(b)
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


def clipped_adam_reference(params, grads, coef, **adam):
    """``params``: CPU fp32 tensors; ``grads``: per step, one CPU fp32 tensor per parameter;
    ``coef``: per step, the fp32 coefficient (or None: that step is skipped, as a
    non-finite norm or a non-zero guard skips it).  Each applied step is
    ``grad * coef`` -- one fp32 multiply, as ``grad.mul_(coef)`` -- then
    torch.optim.Adam(foreach=False).  Returns (params, exp_avg, exp_avg_sq) lists."""
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    opt = torch.optim.Adam(ps, foreach=False, **adam)
    for gs, c in zip(grads, coef):
        if c is None:
            continue
        cf = torch.tensor(float(np.float32(c)), dtype=torch.float32)
        for p, g in zip(ps, gs):
            p.grad = g.detach().clone() * cf
        opt.step()
    st = [opt.state[p] for p in ps]
    return ([p.detach() for p in ps], [s["exp_avg"] if s else torch.zeros_like(p) for s, p in zip(st, ps)],
            [s["exp_avg_sq"] if s else torch.zeros_like(p) for s, p in zip(st, ps)])
