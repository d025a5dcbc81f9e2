"""CPU checks of the clipping reference (tests/clip_ref.py) the GPU tests rest
on: it is torch.nn.utils.clip_grad_norm_ evaluated in float64, IEEE cases
included, and the 1-ulp tolerance of the device norm does not depend on the
order in which the exact squares are summed in double."""
import math

import numpy as np
import pytest
import torch

import clip_ref as C

SHAPES = [(3, 5), (1025,), (7, 9), (1,), (4097,)]


def _grads(seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * (10.0 ** (i % 3 - 1)) for i, s in enumerate(SHAPES)]


def _cases():
    base = _grads()
    n = C.norm64(base)
    inf, nan, both = _grads(), _grads(), _grads()
    inf[1][17] = math.inf
    nan[4][4096] = math.nan
    both[0][1, 2] = math.inf
    both[2][3, 3] = -math.inf
    return {
        "below": (base, 2.0 * n), "above": (base, 0.25 * n), "exactly at": (base, n),
        "max_norm=inf": (base, math.inf), "one inf": (inf, 1.0), "one nan": (nan, 1.0),
        "inf and -inf": (both, 1.0), "inf, max_norm=inf": (inf, math.inf),
        "all zero": ([torch.zeros(s) for s in SHAPES], 1.0), "empty list": ([], 1.0),
    }


CASES = _cases()


@pytest.mark.parametrize("what", sorted(CASES))
def test_reference_is_torch_clip_grad_norm_in_float64(what):
    grads, max_norm = CASES[what]
    ref = C.reference(grads, max_norm)
    ps = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.double().clone()
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False))
    coef = float(torch.clamp(torch.tensor(max_norm, dtype=torch.float64) / (torch.tensor(total, dtype=torch.float64)
                                                                           + 1e-6), max=1.0))
    for mine, theirs in ((ref["norm"], total), (ref["coef"], coef)):
        if math.isnan(theirs) or math.isinf(theirs):
            assert (math.isnan(mine) and math.isnan(theirs)) or mine == theirs, (what, mine, theirs)
        else:
            assert abs(mine - theirs) <= 1e-12 * abs(theirs), (what, mine, theirs)
    assert ref["nonfinite"] == (0 if math.isfinite(total) else 1)
    with np.errstate(invalid="ignore"):
        for p, g in zip(ps, grads):
            want = g.double().numpy() * np.float64(ref["coef"])
            np.testing.assert_allclose(p.grad.numpy(), want, rtol=1e-12, atol=0.0, equal_nan=True)
    # the IEEE cases as include/aaa.h lists them
    if what in ("below", "max_norm=inf", "all zero", "empty list"):
        assert ref["coef"] == 1.0 and ref["stats"][1] == np.float32(1.0)
    if what in ("above", "exactly at"):
        assert ref["coef"] < 1.0
    if what in ("one inf", "inf and -inf"):
        assert ref["coef"] == 0.0 and math.isinf(ref["norm"])
    if what in ("one nan", "inf, max_norm=inf"):
        assert math.isnan(ref["coef"])
    if what in ("all zero", "empty list"):
        assert ref["norm"] == 0.0
    assert C.same_f32(ref["stats"][3], max_norm)


def test_summation_order_in_double_stays_inside_one_fp32_ulp():
    """The GPU tests allow stats[0] 1 fp32 ulp from the rounded fp64 norm.  That
    rests on: any double summation order of the exact squares is within
    N * 2^-53 ~ 2.5e-10 relative of the exact sum, far inside half an fp32 ulp
    (6e-8).  Three different chunkings of the learner-sized vector, elements
    N(0, 1) * 10^k with k uniform in {-3..2} (measured: 0 ulp each)."""
    rng = np.random.default_rng(2270276)
    n = 2_270_276
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
    want = np.float32(C.norm64([g]))
    sq = g.astype(np.float64) ** 2   # exact: 24-bit significands squared fit in 53 bits
    pad = np.concatenate([sq, np.zeros(-n % C.CHUNK)])
    # (a) the kernel's shape: 4096-element chunks, 256 strided lanes each, partials summed in order
    lanes = pad.reshape(-1, 16, 256).sum(axis=1)             # per thread: 16 elements
    a = float(np.cumsum(lanes.sum(axis=1))[-1])
    # (b) 1000-element chunks summed pairwise, partials sequentially
    b = float(np.cumsum(np.add.reduceat(sq, np.arange(0, n, 1000)))[-1])
    # (c) one strictly sequential pass
    c = float(np.cumsum(sq)[-1])
    for name, s in (("chunks of 4096", a), ("chunks of 1000", b), ("sequential", c)):
        got = np.float32(math.sqrt(s))
        print(f"{name}: {C.ulps(got, want)} ulp from the reference")
        assert C.ulps(got, want) <= 1, (name, got, want)


def test_clipped_adam_reference_is_adam_on_the_scaled_gradients():
    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(5, 3, generator=g), torch.randn(17, generator=g)]
    grads = [[torch.randn(p.shape, generator=g) for p in ps] for _ in range(3)]
    coef = [np.float32(0.37), None, np.float32(1.0)]
    got, m, v = C.clipped_adam_reference(ps, grads, coef, lr=1e-3)
    ref = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.Adam(ref, lr=1e-3, foreach=False)
    for gs, c in zip(grads, coef):
        if c is None:
            continue   # a skipped step: neither the moments nor the step count move
        for p, gg in zip(ref, gs):
            p.grad = gg * torch.tensor(float(c))
        opt.step()
    for a, b in zip(got, ref):
        assert torch.equal(a, b.detach())
    assert all(float(opt.state[p]["step"]) == 2.0 for p in ref)
    assert torch.equal(m[0], opt.state[ref[0]]["exp_avg"]) and torch.equal(v[1], opt.state[ref[1]]["exp_avg_sq"])
