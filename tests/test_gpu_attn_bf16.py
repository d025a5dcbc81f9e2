"""The bf16 learner's attention readout kernels, each against fp64 at fp32 accuracy.

aaa_attn_fwd_bf16 / aaa_attn_bwd_bf16 reach the kernels configs 3-5 run and
no fp32-O entry can: the forward k_attn_fwd_mfma<4|8, false, true|false>
(AAA_ATTN_MFMA=1) and k_attn_fwd<4|8, 0|8, 0, __bf16> (=0; the V prefetch from
P > 242), the backward k_attn_bwd<4|8, __bf16, 1|2> (AAA_ATTN_BWD_MFMA=0; two
positions per lane from P > 256) and k_attn_bwd_mfma<4|8> (=2).  O is bf16 in
the learner's [x | h] rows (pitch 192, h at element 64) with the x half and a
spare row filled with a large finite value that must not reach any output.

Per case (inputs, references and bounds: attn_bf16_ref.py):
 a. the project gate: attn, answer, dO, dQ against ref_cpu.attention_readout in
    fp64 on the same values (autograd for the backward) at 1e-4 -- the operands
    are exactly representable, so bf16 excuses nothing wider;
 b. split completeness: the readout columns against the fp64 product of the map
    the kernel returned, and dO[..., :8] / dQ against the explicit fp64 backward
    formulas on the kernel's inputs, within e2 / 2, e2 being the error of that
    quantity with the fp32 operands cut to two bf16 parts.  The MFMA kernels cut
    them to three and must sum every part product; the VALU kernels are plain
    fp32 FMAs.  test_attn_bf16_emulation.py shows fp32 arithmetic within e2 / 4.
    Those e2 are dominated by the operand that reaches all 184 columns (the map,
    the answer gradient), so S has bounds of its own: the forward's basis columns
    with S cut alone, and a backward case whose answer gradient reaches the basis
    columns only.
 c. both settings of each selector in one process give different bits.
"""
import pytest
import torch

import attn_bf16_ref as R
from helpers import assert_close, rel_err

from aaa_amd import _native as N

pytestmark = pytest.mark.gpu
RTOL = 1e-4
F = R.F
QUERY_MODES = ["const_sq", "const", "per_frame"]   # constant Q with sq_scratch / without; per-frame Q


def _o_buffer(c, dev):
    """O in (F*P + 1, 192) bf16 rows, poison in columns 0..63 and in the spare row."""
    buf = torch.full((F * c["P"] + 1, R.O_LD), R.POISON, dtype=torch.bfloat16)
    buf[:F * c["P"], R.O_OFF:] = c["O"].reshape(F * c["P"], 128)
    buf = buf.to(dev)
    return buf, buf.data_ptr() + 2 * R.O_OFF


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _selector(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))


def run_fwd(dev, c, mode):
    nq, P = c["nq"], c["P"]
    buf, optr = _o_buffer(c, dev)
    per_frame = mode == "per_frame"
    assert per_frame == c["per_frame_q"]
    S, pr, pa = (c[k].to(dev) for k in ("S", "pr", "pa"))
    Q = (c["Q"] if per_frame else c["Q"][0]).contiguous().to(dev)
    sq = _nan(dev, P, nq) if mode == "const_sq" else None
    attn, ans = _nan(dev, F, P, nq), _nan(dev, F, 256 * nq + 2)
    N.check(N.load().aaa_attn_fwd_bf16(F, c["h"], c["w"], nq, optr, R.O_LD, S.data_ptr(), Q.data_ptr(),
                                       nq * 72 if per_frame else 0, N.ptr(sq), pr.data_ptr(), pa.data_ptr(),
                                       attn.data_ptr(), ans.data_ptr(), N.stream_ptr()), "attn_fwd_bf16")
    torch.cuda.synchronize()
    return attn.cpu(), ans.cpu()


def check_fwd(c, attn, ans, what):
    nq = c["nq"]
    ro = R.readout64(attn.double(), c["O64"], c["S64"])   # of the map the kernel returned
    e = rel_err(ans[:, :nq * 184].numpy(), ro.numpy())
    es = rel_err(R.s_cols(ans[:, :nq * 184], nq).numpy(), R.s_cols(ro, nq).numpy())
    print(f"{what}: readout vs fp64 of its own map {e:.2e} (e2 {c['fwd_e2']:.2e}), "
          f"basis columns {es:.2e} (e2 {c['fwdS_e2']:.2e})")
    assert_close(attn.numpy(), c["A64"].numpy(), RTOL, what + " attention maps")
    assert_close(ans.numpy(), c["answer64"].numpy(), RTOL, what + " answer")
    assert e <= c["fwd_e2"] / 2, f"{what}: readout error {e:.3e} above e2/2 = {c['fwd_e2'] / 2:.3e}: a bf16 part is lost"
    assert es <= c["fwdS_e2"] / 2, (f"{what}: basis-column error {es:.3e} above e2/2 = {c['fwdS_e2'] / 2:.3e}: "
                                    "a bf16 part of S is lost")
    return e, es


def run_bwd(dev, c, add_q, quad_major, dans_key="dans"):
    nq, P = c["nq"], c["P"]
    buf, optr = _o_buffer(c, dev)
    per_frame = c["per_frame_q"]
    S, A = c["S"].to(dev), c["A32"].contiguous().to(dev)
    Q = (c["Q"] if per_frame else c["Q"][0]).contiguous().to(dev)
    da_ld = 256 * nq + 2 if add_q else nq * 184
    dans = c[dans_key][:, :da_ld].contiguous().to(dev)
    dO, dQ = _nan(dev, F, P * 128), _nan(dev, F, nq, 72)
    N.check(N.load().aaa_attn_bwd_bf16(F, c["h"], c["w"], nq, optr, R.O_LD, S.data_ptr(), Q.data_ptr(),
                                       nq * 72 if per_frame else 0, A.data_ptr(), dans.data_ptr(), da_ld, add_q,
                                       quad_major, dO.data_ptr(), dQ.data_ptr(), N.stream_ptr()), "attn_bwd_bf16")
    torch.cuda.synchronize()
    dO = dO.cpu()
    if quad_major:   # position p, channels 4k..4k+3 at (k*P + p)*4
        dO = dO.reshape(F, 32, P, 4).permute(0, 2, 1, 3)
    return dO.reshape(F, P, 128), dQ.cpu()


def check_bwd(c, dO, dQ, add_q, what):
    nq = c["nq"]
    dq_logits = dQ.double()
    if add_q:   # without the answer row's copy of Q
        dq_logits = dq_logits - c["dans"][:, nq * 184:nq * 256].reshape(F, nq, 72).double()
    errs = (rel_err(dO[:, :, :8].numpy(), c["bwd64"][0].numpy()), rel_err(dq_logits.numpy(), c["bwd64"][1].numpy()))
    print(f"{what}: dO_key {errs[0]:.2e} (e2 {c['bwd_e2'][0]:.2e}), dQ {errs[1]:.2e} (e2 {c['bwd_e2'][1]:.2e})")
    assert_close(dO.numpy(), c["dO64", add_q].numpy(), RTOL, what + " dO")
    assert_close(dQ.numpy(), c["dQ64", add_q].numpy(), RTOL, what + " dQ (per frame)")
    for name, e, e2 in zip(("dO_key", "dQ"), errs, c["bwd_e2"]):
        assert e <= e2 / 2, f"{what}: {name} error {e:.3e} above e2/2 = {e2 / 2:.3e}: a part product of dA is lost"
    return errs


# --------------------------------------------------------------- forward ----
@pytest.mark.parametrize("mode", QUERY_MODES)
@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("nq", R.NQS)
@pytest.mark.parametrize("hw", R.GRIDS)
def test_attn_fwd_bf16_vs_fp64(cuda, monkeypatch, hw, nq, mfma, mode):
    _selector(monkeypatch, "AAA_ATTN_MFMA", mfma)
    c = R.case(hw, nq, mode == "per_frame")
    attn, ans = run_fwd(cuda, c, mode)
    check_fwd(c, attn, ans, f"fwd P={c['P']} nq={nq} mfma={mfma} {mode}")


# -------------------------------------------------------------- backward ----
@pytest.mark.parametrize("per_frame_q", [False, True])
@pytest.mark.parametrize("quad_major", [0, 1])
@pytest.mark.parametrize("add_q", [0, 1])
@pytest.mark.parametrize("mfma", [0, 2])
@pytest.mark.parametrize("nq", R.NQS)
@pytest.mark.parametrize("hw", R.GRIDS)
def test_attn_bwd_bf16_vs_fp64(cuda, monkeypatch, hw, nq, mfma, add_q, quad_major, per_frame_q):
    _selector(monkeypatch, "AAA_ATTN_BWD_MFMA", mfma)
    c = R.case(hw, nq, per_frame_q)
    dO, dQ = run_bwd(cuda, c, add_q, quad_major)
    check_bwd(c, dO, dQ, add_q, f"bwd P={c['P']} nq={nq} mfma={mfma} add_q={add_q} qm={quad_major} pfq={per_frame_q}")


@pytest.mark.parametrize("mfma", [0, 2])
@pytest.mark.parametrize("nq", R.NQS)
@pytest.mark.parametrize("hw", R.BASIS_ONLY_GRIDS)
def test_attn_bwd_bf16_basis_only_gradient_vs_fp64(cuda, monkeypatch, hw, nq, mfma):
    """An answer gradient on the readout's basis columns alone (dA = S da_S^T), the learner's call otherwise:
    in the full case a lost low part of S stays under e2 / 2 (the cut of da dominates that e2); here dO's key
    channels are held to half the error of S cut to two parts."""
    _selector(monkeypatch, "AAA_ATTN_BWD_MFMA", mfma)
    c = R.case(hw, nq, False)
    dO, dQ = run_bwd(cuda, c, 0, 1, "dansS")
    what = f"bwd basis-only P={c['P']} nq={nq} mfma={mfma}"
    e, e2 = rel_err(dO[:, :, :8].numpy(), c["bwdS64"][0].numpy()), c["bwdS_e2"][0]
    print(f"{what}: dO_key {e:.2e} (e2 {e2:.2e}), dQ {rel_err(dQ.numpy(), c['bwdS64'][1].numpy()):.2e} "
          f"(e2 {c['bwdS_e2'][1]:.2e})")
    assert_close(dO.numpy(), c["dO64", "S"].numpy(), RTOL, what + " dO")
    assert_close(dQ.numpy(), c["dQ64", "S"].numpy(), RTOL, what + " dQ (per frame)")
    assert e <= e2 / 2, f"{what}: dO_key error {e:.3e} above e2/2 = {e2 / 2:.3e}: a bf16 part of S is lost in dA"


@pytest.mark.parametrize("nq,hw", [(4, (11, 11)), (8, (21, 21)), (4, (27, 20))])
def test_attn_bf16_default_dispatch_vs_fp64(cuda, monkeypatch, nq, hw):
    """Both selectors unset, the learner's calls: constant query with sq_scratch; add_q 0, quad-major dO."""
    _selector(monkeypatch, "AAA_ATTN_MFMA", None)
    _selector(monkeypatch, "AAA_ATTN_BWD_MFMA", None)
    c = R.case(hw, nq, False)
    attn, ans = run_fwd(cuda, c, "const_sq")
    check_fwd(c, attn, ans, f"fwd P={c['P']} nq={nq} default")
    dO, dQ = run_bwd(cuda, c, 0, 1)
    check_bwd(c, dO, dQ, 0, f"bwd P={c['P']} nq={nq} default")


# ------------------------------------------------------- selector effect ----
def test_attn_fwd_selector_switches_kernel_in_process(cuda, monkeypatch):
    c = R.case((21, 21), 8, False)
    out = {}
    for mfma in (1, 0):
        _selector(monkeypatch, "AAA_ATTN_MFMA", mfma)
        out[mfma] = run_fwd(cuda, c, "const_sq")
        check_fwd(c, *out[mfma], f"fwd selector mfma={mfma}")
    assert not torch.equal(out[1][1], out[0][1]), "AAA_ATTN_MFMA=0 and 1 gave bit-identical answers: one kernel ran twice"


def test_attn_bwd_selector_switches_kernel_in_process(cuda, monkeypatch):
    c = R.case((21, 21), 8, False)
    out = {}
    for mfma in (2, 0):
        _selector(monkeypatch, "AAA_ATTN_BWD_MFMA", mfma)
        out[mfma] = run_bwd(cuda, c, 0, 1)
        check_bwd(c, *out[mfma], 0, f"bwd selector mfma={mfma}")
    same = torch.equal(out[2][0], out[0][0]) and torch.equal(out[2][1], out[0][1])
    assert not same, "AAA_ATTN_BWD_MFMA=0 and 2 gave bit-identical dO and dQ: one kernel ran twice"
