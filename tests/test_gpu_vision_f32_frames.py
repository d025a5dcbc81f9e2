"""The frame-resident fp32 (split-product) vision encoder forward, k_vision_fwd_f32
(csrc/vision_f32.h), through the checker entry aaa_vision_enc_f32_fwd (runtime.py
EncF32Runner), which calls the learner's own dispatch (vision_fwd<float, float>) and hands
back the raw products: the fp32 bordered frames Xp, conv1's Y1 and conv2's output rows.

Bounds (tests/f32_split_ref.py; CPU evidence: tests/test_vision_f32_frames_emulation.py): each
conv against fp64 on the kernel's OWN operands within e2 / 2, e2 = the error of that conv with
one operand cut to two bf16 parts.  uint8 frames are exact in bf16, so conv1's input site is
bounded with scaled fp32 frames only.  Reference: attention.py:155-170 on X.transpose(1,3) (:179)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f32_split_ref as R
from helpers import assert_close, detinit, rel_err
from test_gpu_parity import RTOL, _agent, _compare, _cot, _grads, _oracle

import attention

pytestmark = pytest.mark.gpu
N = attention._pkg._native
RT = attention._pkg.runtime
PARAMS = detinit.deterministic_params(0, 18)
KEYS = [R.CNN + k for k in ("0.weight", "0.bias", "1.weight", "1.bias")]
FUSED = "k_vision_fwd_f32"


def _flat(dev):
    return torch.cat([torch.as_tensor(np.ascontiguousarray(PARAMS[k])).float().reshape(-1) for k in KEYS]).to(dev)


def _frames_u8(n, H, W):
    return torch.from_numpy(detinit.frames_u8(1234, (1, n, H, W, 3)))[0]


def _run(cuda, frames, out_ld=192):
    """One forward: (xp, y1, out) on the host and the timer's variant."""
    n, H, W, _ = frames.shape
    enc = RT.EncF32Runner(n, H, W, out_ld=out_ld, frames_u8=frames.dtype == torch.uint8, device=cuda)
    flat = _flat(cuda)
    packed = enc.pack(flat)
    N.timing_enable(True)
    try:
        xp, y1, out = enc.forward(flat, packed, frames.to(cuda))
        torch.cuda.synchronize()
        st = N.timing_stats(N.TIMER_VISION_FWD)
    finally:
        N.timing_enable(False)
    return enc, xp.cpu(), y1.cpu(), out.cpu(), st["variant"]


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _e2(x, y1k, sites1):
    """f32_split_ref.cnn_e2's forward half alone (cnn_pieces' formulas; the backward products are not computed:
    the CUs + 3 case has 259 frames): fp64 conv1 of x and conv2 of the kernel's own y1, and e2 per site."""
    w1, b1, w2, b2 = R.cnn_weights(PARAMS)
    x, y1k = x.double(), y1k.double()
    c1 = lambda xx, ww: F.conv2d(xx, ww, b1, stride=4, padding=1)    # noqa: E731
    c2 = lambda yy, ww: F.conv2d(yy, ww, b2, stride=2, padding=2)    # noqa: E731
    ex = {"y1": c1(x, w1), "y2": c2(y1k, w2)}
    cut = {"conv1.W": lambda: c1(x, R._cut(w1)), "conv1.x": lambda: c1(R._cut(x), w1)}
    e2 = {(s, "y1"): rel_err(cut[s](), ex["y1"]) for s in sites1}
    e2["conv2.W", "y2"] = rel_err(c2(y1k, R._cut(w2)), ex["y2"])
    e2["conv2.y1", "y2"] = rel_err(c2(R._cut(y1k), w2), ex["y2"])
    return ex, e2


def _check(what, frames, xp, y1, out, sites1):
    """Accuracy on the kernel's own operands, everything written, nothing else touched."""
    n, H, W, _ = frames.shape
    fr = frames.float()
    # 2. Xp = float(frame) bit for bit, zero border, zero channel 3; no NaN left; columns 64.. keep the sentinel
    exp = torch.zeros(n, H + 2, W + 2, 4)
    exp[:, 1:-1, 1:-1, :3] = fr
    assert torch.equal(xp.view(torch.int32), exp.view(torch.int32)), f"{what}: Xp is not float(frame), zero-bordered"
    assert not torch.isnan(y1).any(), f"{what}: Y1 has unwritten elements"
    if out.shape[2] > 64:
        assert bool((out[:, :, 64:].contiguous().view(torch.int32) == RT.EncF32Runner.SENTINEL).all()), \
            f"{what}: columns 64.. were written"
    # 1. each conv against fp64 on its own operands
    nhwc = lambda t: t.permute(0, 3, 2, 1).contiguous()   # noqa: E731
    h, w = R.ref_cpu.grid_of(H, W)
    ex, e2 = _e2(nhwc(fr), nhwc(y1), sites1)
    got = {"y1": nhwc(y1), "y2": nhwc(out[:, :, :64].reshape(n, h, w, 64))}
    bad = []
    for obs, sites in (("y1", sites1), ("y2", ("conv2.W", "conv2.y1"))):
        err = rel_err(got[obs], ex[obs])
        for s in sites:
            print(f"{what}: {obs} err {err:.3e}, e2[{s}] {e2[s, obs]:.3e}, err / e2 {err / e2[s, obs]:.3f}")
            if not err <= e2[s, obs] / 2:
                bad.append((what, obs, s, err, e2[s, obs]))
    assert not bad, bad


@pytest.mark.parametrize("case", ["2x84x84", "5x64x64", "cus+3"])
def test_u8_accuracy_on_own_operands(cuda, case):
    """(2,84,84); (5,64,64): P1 = 225 and P = 64, ragged column blocks in both convs; (CUs+3,84,84): more than one
    frame per workgroup and a ragged last round."""
    n, H, W = {"2x84x84": (2, 84, 84), "5x64x64": (5, 64, 64), "cus+3": (_cus() + 3, 84, 84)}[case]
    fr = _frames_u8(n, H, W)
    _, xp, y1, out, var = _run(cuda, fr)
    assert FUSED in var, var
    _check(f"u8 {case}", fr, xp, y1, out, ("conv1.W",))
    assert N.pair_status(clear=True) == 0


def test_f32_frames_accuracy_on_own_operands(cuda):
    """Scaled fp32 frames (x 0.37): conv1's input site is live."""
    fr = _frames_u8(2, 84, 84).float() * R.FRAME_SCALE
    _, xp, y1, out, var = _run(cuda, fr)
    assert FUSED in var, var
    _check("f32 2x84x84", fr, xp, y1, out, ("conv1.W", "conv1.x"))


@pytest.mark.parametrize("n,H,W", [(2, 84, 84), (5, 64, 64)])
def test_u8_equals_f32_frames(cuda, n, H, W):
    fr = _frames_u8(n, H, W)
    a = _run(cuda, fr)
    b = _run(cuda, fr.float())
    assert FUSED in a[4] and FUSED in b[4], (a[4], b[4])
    for x, y, name in zip(a[1:4], b[1:4], ("xp", "y1", "out")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{name}: uint8 and fp32 frames differ"


def test_plain_output_pitch(cuda):
    """out_ld = 64 (the component entry's): every column written."""
    fr = _frames_u8(2, 84, 84)
    _, xp, y1, out, var = _run(cuda, fr, out_ld=64)
    assert FUSED in var, var
    ref = _run(cuda, fr)[3]
    assert torch.equal(out, ref[:, :, :64].contiguous())


def _learner(cuda, T, B, H=84, W=84, grid=(11, 11)):
    """One learner unroll + backward on uint8 frames -> (outputs, grads, the vision forward's variant)."""
    X = torch.from_numpy(detinit.frames_u8(1234, (T, B, H, W, 3))).to(cuda)
    Gl, Gv = (g.to(cuda) for g in _cot(T, B))
    ag = _agent(cuda, grid=grid)
    ag.reset()
    N.timing_enable(True)
    try:
        lg, vl, at = ag.unroll(X)
        torch.cuda.synchronize()
        var = N.timing_stats(N.TIMER_VISION_FWD)["variant"]
    finally:
        N.timing_enable(False)
    ((lg * Gl).sum() + (vl * Gv).sum()).backward()
    torch.cuda.synchronize()
    return (lg.detach().cpu(), vl.detach().cpu(), at.detach().cpu(), _grads(ag)), var


def test_dispatch(cuda, monkeypatch):
    monkeypatch.delenv("AAA_VIS_FRAMES", raising=False)
    fused, var = _learner(cuda, 2, 2)
    assert FUSED in var, var
    monkeypatch.setenv("AAA_VIS_FRAMES", "0")
    layered, var0 = _learner(cuda, 2, 2)
    assert "layered" in var0 and FUSED not in var0, var0
    for a, b, name in zip(fused[:2], layered[:2], ("logits", "values")):
        assert_close(a.numpy(), b.numpy(), RTOL, f"fused vs layered {name}")
    for name in fused[3]:
        if float(layered[3][name].norm()) > 0:
            assert_close(fused[3][name].numpy(), layered[3][name].numpy(), RTOL, f"fused vs layered grad {name}")
    monkeypatch.delenv("AAA_VIS_FRAMES", raising=False)
    h, w = N.grid(210, 160)
    _, var = _learner(cuda, 1, 1, 210, 160, grid=(h, w))
    assert "layered" in var, var   # vis_fits is false


def test_packed_weights(cuda):
    """hi + mid + lo of each pre-split region, un-permuted, is the fp32 weight within 2^-23."""
    enc = RT.EncF32Runner(1, 84, 84, device=cuda)
    packed = enc.pack(_flat(cuda)).cpu()
    n1, n2 = 16 * 3 * 64 * 16, 2 * 32 * 3 * 64 * 16
    w1 = torch.as_tensor(np.ascontiguousarray(PARAMS[KEYS[0]])).float()   # (32,3,kx,ky)
    w2 = torch.as_tensor(np.ascontiguousarray(PARAMS[KEYS[2]])).float()   # (64,32,kx,ky)
    W1 = torch.zeros(32, 8, 8, 4)
    W1[..., :3] = w1.permute(0, 3, 2, 1)
    regions = (("conv1", packed[-(n1 + n2):-n2], 1, 16, W1.reshape(32, 256)),
               ("conv2", packed[-n2:], 2, 32, w2.permute(0, 3, 2, 1).reshape(64, 512)))
    for name, raw, nrb, nks, want in regions:
        parts = raw.contiguous().view(torch.bfloat16).reshape(nrb, nks, 3, 2, 32, 8)
        parts = parts.permute(2, 0, 4, 1, 3, 5).reshape(3, nrb * 32, nks * 16).double()
        got = parts.sum(0)
        nz = want != 0
        rel = ((got - want.double()).abs()[nz] / want.double().abs()[nz]).max()
        print(f"{name}: hi + mid + lo against the fp32 weight, worst relative {float(rel):.3e}")
        assert float(rel) <= 2.0 ** -23, (name, float(rel))
        assert torch.equal(got[~nz], torch.zeros_like(got[~nz]))
        assert bool((parts[2] != 0).any()), f"{name}: the lo plane is all zero"


def test_end_to_end_vs_oracle(cuda, monkeypatch):
    monkeypatch.delenv("AAA_VIS_FRAMES", raising=False)
    out, var = _learner(cuda, 3, 2)
    assert FUSED in var, var
    _compare(out, _oracle(3, 2), RTOL, "fused fp32 encoder T=3 B=2: ")
    assert N.pair_status(clear=True) == 0
