"""The float64 statements of the V-trace actor-critic loss that the device
kernel is held against (tests/vtrace_ref.py), checked on the CPU: the autograd
statement and the literal per-step loop agree, the targets reduce to the
discounted n-step return where V-trace says they must, and the inputs the GPU
tests use exercise both sides of every importance-ratio clip."""
import pytest
import torch

import vtrace_ref as R

IDS = [R.case_id(c) for c in R.CASES]


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_autograd_and_literal_statements_agree(i):
    c = R.CASES[i]
    x, hp = R.case_inputs(i), R.case_hparams(c)
    a, b = R.reference(**x, **hp), R.literal(**x, **hp)
    for k in ("dlogits", "dvalues", "vs", "pg_adv", "parts", "loss"):
        err = float((a[k] - b[k]).abs().max())
        assert err <= 1e-12 * max(1.0, float(a[k].abs().max())), (k, err)
    off = torch.ones(c["A"], dtype=torch.bool)
    off[c["vc"]] = False
    assert float(a["dvalues"][..., off].abs().max()) == 0.0 == float(b["dvalues"][..., off].abs().max())


@pytest.mark.parametrize("boot", [True, False])
def test_on_policy_lambda_one_is_the_n_step_return(boot):
    T, B, A, gamma = 23, 4, 6, 0.9
    x = R.make_inputs(T, B, A, 77, mu=False, done=False, boot=boot)
    out = R.reference(**x, gamma=gamma, lam=1.0)
    VT = x["bootstrap"].double() if boot else torch.zeros(B, dtype=torch.float64)
    ret, G = [None] * T, VT
    for t in range(T - 1, -1, -1):
        G = x["rewards"][t].double() + gamma * G
        ret[t] = G
    ret = torch.stack(ret)
    assert float((out["vs"] - ret).abs().max()) <= 1e-12 * float(ret.abs().max())
    # ... and the policy-gradient advantage is that return's one-step form minus the baseline
    nxt = torch.cat([ret[1:], VT[None]])
    adv = x["rewards"].double() + gamma * nxt - x["values"][..., 0].double()
    assert float((out["pg_adv"] - adv).abs().max()) <= 1e-12 * float(adv.abs().max())


def test_done_cuts_the_return():
    T, B, A = 9, 2, 4
    x = R.make_inputs(T, B, A, 5, done=False)
    done = torch.zeros(T, B)
    done[3, 1] = 1.0
    y = {k: (v.clone() if v is not None else None) for k, v in x.items()}
    for k in ("logits", "values", "rewards"):
        y[k][4:, 1] += 1.0
    a, b = R.reference(**dict(x, done=done)), R.reference(**dict(y, done=done))
    for k in ("dlogits", "dvalues", "vs", "pg_adv"):
        assert torch.equal(a[k][:4, 1], b[k][:4, 1]), k
        assert torch.equal(a[k][:, 0], b[k][:, 0]), k


@pytest.mark.parametrize("i", [i for i, c in enumerate(R.CASES) if c["mu"]],
                         ids=[R.case_id(c) for c in R.CASES if c["mu"]])
def test_gpu_inputs_exercise_both_sides_of_each_clip(i):
    """With the behaviour log-probs from independent logits, between 10 % and
    90 % of the (t, b) have e^{log rho} above each clip the case uses.  The
    (1, 1, 2) case has a single (t, b), of which no fraction lies strictly
    between: there only the ratio's finiteness is asserted (both sides of the
    clips are exercised by every other case)."""
    c = R.CASES[i]
    ratio = R.ratios(R.case_inputs(i))
    assert bool(torch.isfinite(ratio).all()) and float(ratio.min()) > 0.0
    if ratio.numel() == 1:
        return
    hp = R.case_hparams(c)
    for bar in ("rho_bar", "c_bar", "pg_rho_bar"):
        frac = float((ratio > hp[bar]).double().mean())
        assert 0.1 <= frac <= 0.9, (bar, hp[bar], frac)
