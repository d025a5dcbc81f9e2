"""CPU checks of the RMSProp reference (tests/rmsprop_ref.py) the GPU tests rest
on: it is ``torch.optim.RMSprop`` evaluated in float64, its eps-inside-the-root
form is the element worked by hand, the schedule is the linear anneal clamped
at ``lr_end``, and a skipped step moves neither the state nor the schedule."""
import math

import numpy as np
import pytest
import torch

import rmsprop_ref as R

SHAPES = [(3, 5), (1025,), (7, 9), (1,), (4097,)]
CASES = {
    "plain": dict(lr=1e-2),
    "weight_decay": dict(lr=3e-3, weight_decay=0.01),
    "momentum": dict(lr=1e-3, momentum=0.9),
    "centered": dict(lr=1e-3, centered=True),
    "centered + momentum": dict(lr=1e-3, centered=True, momentum=0.9, eps=1e-5),
    "maximize": dict(lr=1e-3, alpha=0.9, eps=1e-6, maximize=True),
}


def _inputs(seed=11, steps=4):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) * (10.0 ** ((i + k) % 3 - 1)) for i, s in enumerate(SHAPES)]
             for k in range(steps)]
    return ps, grads


@pytest.mark.parametrize("what", sorted(CASES))
def test_statement_is_torch_rmsprop_in_float64(what):
    hp = CASES[what]
    ps, grads = _inputs()
    ref = R.run(ps, grads, **hp)
    tp = [p.double().clone().requires_grad_(True) for p in ps]
    opt = torch.optim.RMSprop(tp, foreach=False, **hp)
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = g.double().clone()
        opt.step()
    full = dict(R.DEFAULTS, **hp)
    for i, p in enumerate(tp):
        np.testing.assert_allclose(ref["params"][i], p.detach().numpy(), rtol=1e-12, atol=1e-12)
        assert set(opt.state[p]) - {"step"} == set(R.used(full))
        for k in R.used(full):
            np.testing.assert_allclose(ref[k][i], opt.state[p][k].numpy(), rtol=1e-12, atol=1e-12)
    for k in R.STATE:
        assert (ref[k] is None) == (k not in R.used(full))
    assert ref["applied"] == len(grads)


def test_eps_in_sqrt_against_a_hand_evaluated_element():
    # p = 1, g = 2, v0 = 0, alpha = 0.75, eps = 0.25:  v = 0.25 * 4 = 1
    #   inside the root:  avg = sqrt(1.25),     p = 1 - 0.5 * 2 / sqrt(1.25)
    #   outside (torch):  avg = sqrt(1) + 0.25, p = 1 - 0.5 * 2 / 1.25
    kw = dict(lr=0.5, alpha=0.75, eps=0.25)
    p, g = [np.array([1.0])], [[np.array([2.0])]]
    inside = R.run(p, g, eps_in_sqrt=True, **kw)
    outside = R.run(p, g, eps_in_sqrt=False, **kw)
    assert inside["square_avg"][0][0] == 1.0 and outside["square_avg"][0][0] == 1.0
    assert abs(inside["params"][0][0] - (1.0 - 1.0 / math.sqrt(1.25))) < 1e-15
    assert abs(outside["params"][0][0] - (1.0 - 1.0 / 1.25)) < 1e-15
    # a second step, with momentum: b1 = 2 / sqrt(1.25); v = 0.75 + 0.25 * 9 = 3; b2 = 0.5 * b1 + 3 / sqrt(3.25)
    two = R.run(p, [[np.array([2.0])], [np.array([3.0])]], eps_in_sqrt=True, momentum=0.5, **kw)
    b1 = 2.0 / math.sqrt(1.25)
    b2 = 0.5 * b1 + 3.0 / math.sqrt(3.25)
    assert abs(two["momentum_buffer"][0][0] - b2) < 1e-15
    assert abs(two["params"][0][0] - (1.0 - 0.5 * b1 - 0.5 * b2)) < 1e-15


def test_schedule():
    lr, end, n = 6e-4, 1e-4, 8
    assert R.schedule(0, lr, end, n) == lr
    assert abs(R.schedule(4, lr, end, n) - 3.5e-4) < 1e-18
    assert abs(R.schedule(2, lr, end, n) - (end + (lr - end) * 0.75)) < 1e-18
    assert R.schedule(n, lr, end, n) == end
    assert R.schedule(n + 1, lr, end, n) == end and R.schedule(10 ** 9, lr, end, n) == end
    assert R.schedule(n, lr, 0.0, n) == 0.0 and R.schedule(3 * n, lr, 0.0, n) == 0.0
    assert R.schedule(5, lr, end, 0) == lr and R.schedule(10 ** 9, lr) == lr   # 0: constant
    assert [R.schedule(k, 1.0, 0.0, 4) for k in range(6)] == [1.0, 0.75, 0.5, 0.25, 0.0, 0.0]
    # the package's own statement of it (Learner.current_lr) is the same function
    from helpers import ROOT  # noqa: F401  (path setup)
    import attention  # noqa: F401
    from aaa_amd.optim import rmsprop_lr
    for k in (0, 1, 4, 7, 8, 9):
        assert rmsprop_lr(k, lr, end, n) == R.schedule(k, lr, end, n)
    assert rmsprop_lr(5, lr) == lr


def test_a_skipped_step_leaves_the_state_and_the_schedule_in_place():
    ps, grads = _inputs(steps=5)
    hp = dict(lr=1e-2, lr_end=1e-3, anneal_steps=4, momentum=0.9, centered=True)
    skip = [False, True, False, True, False]
    got = R.run(ps, grads, skip=skip, **hp)
    only = R.run(ps, [grads[0], grads[2], grads[4]], **hp)
    assert got["applied"] == 3 and got["lrs"] == only["lrs"] == [R.schedule(k, 1e-2, 1e-3, 4) for k in range(3)]
    for k in ("params",) + R.STATE:
        for a, b in zip(got[k], only[k]):
            assert np.array_equal(a, b)
    # a run continued from a saved state is the run itself
    first = R.run(ps, grads[:2], **hp)
    rest = R.run(first["params"], grads[2:], state=first, applied=first["applied"], **hp)
    whole = R.run(ps, grads, **hp)
    for k in ("params",) + R.STATE:
        for a, b in zip(rest[k], whole[k]):
            assert np.array_equal(a, b)
    assert rest["applied"] == 5
    # all skipped: nothing moves
    none = R.run(ps, grads, skip=[True] * 5, **hp)
    assert none["applied"] == 0 and all(np.array_equal(a, b.double().numpy()) for a, b in zip(none["params"], ps))
    assert all(not v.any() for v in none["square_avg"])


def test_clip_coefficient_is_one_fp32_multiply():
    ps, grads = _inputs(steps=1)
    c = np.float32(0.37)
    got = R.run(ps, grads, coef=[c], lr=1e-2)
    want = R.run(ps, [[g * torch.tensor(float(c)) for g in grads[0]]], lr=1e-2)
    for a, b in zip(got["params"], want["params"]):
        assert np.array_equal(a, b)
    same = R.run(ps, grads, coef=[np.float32(1.0)], lr=1e-2)
    plain = R.run(ps, grads, lr=1e-2)
    assert all(np.array_equal(a, b) for a, b in zip(same["params"], plain["params"]))


def test_torch_fp32_restatement_tracks_the_statement():
    """What the GPU tolerance's second term measures: fp32 in torch's op order against the
    statement, here on small tensors.  The bound is counted, not measured: at most 12 fp32
    roundings (2^-24 each) per element and step, 4 steps, accumulating at most linearly --
    2.9e-6 relative to the tensor's largest element; the centered variance v - a^2 keeps at
    least alpha^4 = 0.96 of v after 4 steps from zero state, so its subtraction amplifies
    that by under 1.05.  1e-5 leaves a factor of three."""
    ps, grads = _inputs()
    for what, hp in sorted(CASES.items()):
        ref, t32 = R.run(ps, grads, **hp), R.torch_fp32(ps, grads, **hp)
        d = max(R.distance(a, b) for k in ("params",) + R.used(dict(R.DEFAULTS, **hp)) for a, b in zip(t32[k], ref[k]))
        print(f"{what}: torch fp32 CPU is {d:.2e} from the float64 statement")
        assert d < 1e-5, (what, d)
