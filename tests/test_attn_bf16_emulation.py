"""The precondition of test_gpu_attn_bf16.py's split-completeness check, on the
CPU over its whole matrix: the error ``e2`` of a readout / dA product whose
fp32 operands keep only two of their three bf16 parts (attn_bf16_ref.py) is a
few 1e-6, and plain fp32 arithmetic of the same quantity on the same inputs
sits within e2 / 4 -- so a bound of e2 / 2 on a kernel that claims "fp32 FMAs
up to summation order" has a 2x margin on either side: a kernel missing a low
part lands at about e2, a complete one at fp32 summation noise."""
import pytest
import torch

import attn_bf16_ref as R


def test_split2_is_two_bf16_parts():
    x = R.rnd((4096,), 7)
    hi = x.to(torch.bfloat16)
    two = R.split2(x)
    err = ((two - x.double()).abs() / x.double().abs().clamp_min(1e-30)).max()
    assert 2.0 ** -20 < float(err) <= 2.0 ** -16   # two round-to-nearest cuts to 8 significand bits: 2^-8 each
    lo = (x - hi.float() - (x - hi.float()).to(torch.bfloat16).float()).to(torch.bfloat16)
    assert torch.equal(two + lo.double(), x.double())   # hi + mid + lo is the fp32 value exactly


@pytest.mark.parametrize("per_frame_q", [False, True])
@pytest.mark.parametrize("nq", R.NQS)
@pytest.mark.parametrize("hw", R.GRIDS)
def test_fp32_arithmetic_sits_within_a_quarter_of_e2(hw, nq, per_frame_q):
    c = R.case(hw, nq, per_frame_q)
    print(f"P={c['P']} nq={nq} fwd e2 {c['fwd_e2']:.2e} fp32 {c['fwd_f32']:.2e} | bwd dO_key e2 {c['bwd_e2'][0]:.2e} "
          f"fp32 {c['bwd_f32'][0]:.2e} | dQ e2 {c['bwd_e2'][1]:.2e} fp32 {c['bwd_f32'][1]:.2e}")
    # a missing part is far inside the project's 1e-4 gate and far above fp32 noise
    print(f"    fwd basis columns, S cut alone: e2 {c['fwdS_e2']:.2e} fp32 {c['fwdS_f32']:.2e}")
    for e2 in (c["fwd_e2"],) + c["bwd_e2"]:
        assert 5e-7 < e2 < 2e-5, e2
    # (the 3x5 basis is mostly short binary fractions, cos(k pi / 3): its low parts carry little)
    assert (2e-7 if hw == (3, 5) else 5e-7) < c["fwdS_e2"] < 2e-5, c["fwdS_e2"]
    assert c["fwd_f32"] <= c["fwd_e2"] / 4, (c["fwd_f32"], c["fwd_e2"])
    assert c["fwdS_f32"] <= c["fwdS_e2"] / 4, (c["fwdS_f32"], c["fwdS_e2"])
    for name, f32, e2 in zip(("dO_key", "dQ"), c["bwd_f32"], c["bwd_e2"]):
        assert f32 <= e2 / 4, (name, f32, e2)
    print(f"    bwd, basis-only gradient, S cut alone: dO_key e2 {c['bwdS_e2'][0]:.2e} fp32 {c['bwdS_f32'][0]:.2e} | "
          f"dQ e2 {c['bwdS_e2'][1]:.2e} fp32 {c['bwdS_f32'][1]:.2e}")
    # held on dO_key and off the 3x5 grid only (attn_bf16_ref.BASIS_ONLY_GRIDS): the 3x5 basis has next to no
    # low part to lose (e2 within 2x of fp32 arithmetic), and dQ's own fp32 sum over the positions sits at
    # e2 / 4 in places -- dO_key = dlogit Q[:, :8] carries the same dA
    if hw in R.BASIS_ONLY_GRIDS:
        assert 5e-7 < c["bwdS_e2"][0] < 2e-5, c["bwdS_e2"][0]
        assert c["bwdS_f32"][0] <= c["bwdS_e2"][0] / 4, (c["bwdS_f32"][0], c["bwdS_e2"][0])
