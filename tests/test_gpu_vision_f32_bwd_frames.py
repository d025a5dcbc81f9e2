"""The frame-resident fp32 (split-product) vision encoder backward, k_vision_bwd_f32
(csrc/vision_bwd_f32.h), through the checker entry aaa_vision_enc_f32_bwd (runtime.py
EncF32Runner.backward), which calls the learner's own dispatch (vision_bwd_alone<float>) and
hands back the packed gradients and the fp32 dY1 the kernel committed on chip.

Inputs: uint8 frames, the kernel's own forward Y1, a seeded dY2.  Bounds (tests/f32_split_ref.py
cnn_pieces / cnn_e2, CNN_REACH; CPU evidence: tests/test_vision_f32_bwd_frames_emulation.py): each
product against fp64 on the kernel's OWN operands within e2 / 2, e2 = the error of that product with
one operand cut to two bf16 parts -- a kernel that lost a lo part at a site sits AT e2 of that site,
so the bound also shows every lo plane live.  wgrad1.x is invisible on integer frames (exact in bf16),
as conv1.x is in the forward test.  gb1 (a plain fp32 column sum) within test_gpu_parity's RTOL."""
import functools

import numpy as np
import pytest
import torch

import f32_split_ref as R
from helpers import assert_close, detinit, rel_err
from test_gpu_parity import RTOL, _agent, _compare, _cot, _grads, _oracle

import attention

pytestmark = pytest.mark.gpu

N = attention._pkg._native
RT = attention._pkg.runtime
PARAMS = detinit.deterministic_params(0, 18)
KEYS = [R.CNN + k for k in ("0.weight", "0.bias", "1.weight", "1.bias")]
FUSED = "k_vision_bwd_f32"
SITES = {"dy1": ("dgrad2.W", "dgrad2.dy2"), "gW2": ("wgrad2.y1", "wgrad2.dy2"), "gW1": ("wgrad1.dy1",)}
N1, N2 = 32 * 3 * 64, 64 * 32 * 16   # conv1 / conv2 weight elements of the flat gradient


@pytest.fixture(autouse=True)
def _small_frame_counts_fuse(monkeypatch):
    """AAA_VBWD_MINF's fp32 default (1 frame per CU) keeps a handful of frames on the layered launches, which are
    faster there; the cases below are small on purpose, so they lift the floor.  test_default_floor pins the default."""
    monkeypatch.setenv("AAA_VBWD_MINF", "0")


def _flat(dev):
    return torch.cat([torch.as_tensor(np.ascontiguousarray(PARAMS[k])).float().reshape(-1) for k in KEYS]).to(dev)


def _frames_u8(n, H, W):
    return torch.from_numpy(detinit.frames_u8(1234, (1, n, H, W, 3)))[0]


def _nhwc(t):
    return t.permute(0, 3, 2, 1).contiguous()   # (N, H, W, C) -> the reference's (N, C, W, H)


def _run(cuda, frames, dy2, max_groups=0):
    """Forward, then one backward -> (y1, grads, dy1, fused, variant) on the host."""
    n, H, W, _ = frames.shape
    enc = RT.EncF32Runner(n, H, W, frames_u8=frames.dtype == torch.uint8, device=cuda)
    flat = _flat(cuda)
    packed = enc.pack(flat)
    fr = frames.to(cuda)
    xp, y1, _ = enc.forward(flat, packed, fr)
    N.timing_enable(True)
    try:
        grads, dy1, fused = enc.backward(packed, fr, dy2.to(cuda), y1, xp, max_groups=max_groups)
        torch.cuda.synchronize()
        var = N.timing_stats(N.TIMER_VISION_BWD)["variant"]
    finally:
        N.timing_enable(False)
    return y1.cpu(), grads.cpu(), dy1.cpu(), fused, var


def _dy2(n, H, W, seed=7):
    h, w = R.ref_cpu.grid_of(H, W)
    return R.rnd((n, h * w, 64), seed)


def _split(grads):
    return {"gW1": grads[:N1].reshape(32, 3, 8, 8), "gb1": grads[N1:N1 + 32],
            "gW2": grads[N1 + 32:N1 + 32 + N2].reshape(64, 32, 4, 4), "gb2": grads[N1 + 32 + N2:]}


def _check(what, frames, dy2, y1, grads, dy1):
    """Each observable against fp64 on the kernel's own operands, within e2 / 2 of each live site."""
    n, H, W, _ = frames.shape
    h, w = R.ref_cpu.grid_of(H, W)
    assert not torch.isnan(dy1).any(), f"{what}: dY1 has unwritten elements"
    W64 = R.cnn_weights(PARAMS)
    ex, e2 = R.cnn_e2(W64, _nhwc(frames.float()), _nhwc(dy2.reshape(n, h, w, 64)), _nhwc(y1), _nhwc(dy1))
    got = dict(_split(grads), dy1=_nhwc(dy1))
    bad = []
    for obs, sites in SITES.items():
        err = rel_err(got[obs], ex[obs])
        for s in sites:
            print(f"{what}: {obs} err {err:.3e}, e2[{s}] {e2[s, obs]:.3e}, err / e2 {err / e2[s, obs]:.3f}")
            if not err <= e2[s, obs] / 2:
                bad.append((what, obs, s, err, e2[s, obs]))
    assert not bad, bad
    assert_close(got["gb1"].numpy(), ex["gb1"].numpy(), RTOL, f"{what}: gb1")
    assert_close(got["gb2"].numpy(), ex["gb2"].numpy(), RTOL, f"{what}: gb2")


@pytest.mark.parametrize("case", ["2x84x84", "5x64x64", "5x84x84-groups2"])
def test_accuracy_on_own_operands(cuda, case):
    """(2,84,84); (5,64,64): P1 = 225 and P = 64, ragged column blocks and a ragged K step in both weight
    gradients; (5,84,84) on two workgroups: 3 + 2 frames, accumulators carried across frames, a ragged last round.
    Two runs are bit-identical (no atomics)."""
    n, H, W, mg = {"2x84x84": (2, 84, 84, 0), "5x64x64": (5, 64, 64, 0), "5x84x84-groups2": (5, 84, 84, 2)}[case]
    fr, dy2 = _frames_u8(n, H, W), _dy2(n, H, W)
    y1, grads, dy1, fused, var = _run(cuda, fr, dy2, mg)
    assert fused and FUSED in var, var
    _check(case, fr, dy2, y1, grads, dy1)
    _, grads2, dy1b, fused2, _ = _run(cuda, fr, dy2, mg)
    assert fused2
    for k in ("gW2", "gW1", "gb1"):   # the kernel's products (gb2 is the entry's column sum of dY2, by atomics)
        assert torch.equal(_split(grads)[k].view(torch.int32), _split(grads2)[k].view(torch.int32)), f"two runs differ: {k}"
    assert torch.equal(dy1.view(torch.int32), dy1b.view(torch.int32)), "two runs differ: dY1"
    assert N.pair_status(clear=True) == 0


def test_single_pixel(cuda):
    """One nonzero of dY2 at a corner pixel (frame 0) and one in the interior (frame 1): a wrong tap or parity
    mapping, which smooth data averages away, moves whole entries here (values with three nonzero bf16 parts)."""
    n, H, W = 2, 84, 84
    h, w = R.ref_cpu.grid_of(H, W)
    fr = _frames_u8(n, H, W)
    dy2 = torch.zeros(n, h * w, 64)
    dy2[0, 0, 5] = 1.2345678
    dy2[1, 4 * w + 6, 37] = -0.7654321
    y1, grads, dy1, fused, var = _run(cuda, fr, dy2)
    assert fused and FUSED in var, var
    _check("single pixel", fr, dy2, y1, grads, dy1)
    # the support of dY1: exactly the pixels conv2's 4x4 stride-2 pad-2 window of that output pixel covers
    W64 = R.cnn_weights(PARAMS)
    ex = R.cnn_pieces(W64, _nhwc(fr.float()), _nhwc(dy2.reshape(n, h, w, 64)), _nhwc(y1))
    assert torch.equal(_nhwc(dy1) != 0, ex["dy1"] != 0), "dY1's support differs from the reference's"


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same(what, a, b):
    for k, x in _split(a[1]).items():
        assert_close(x.numpy(), _split(b[1])[k].numpy(), RTOL, f"{what}: {k}")
    assert_close(a[2].numpy(), b[2].numpy(), RTOL, f"{what}: dy1")


def test_more_frames_than_cus_against_layered(cuda, monkeypatch):
    """(CUs + 3, 84, 84) with the default grid: two rounds, the last one ragged, against the layered launches."""
    monkeypatch.delenv("AAA_VIS_BWD_FRAMES", raising=False)
    monkeypatch.delenv("AAA_VBWD_MINF", raising=False)   # every default
    n = _cus() + 3
    fr, dy2 = _frames_u8(n, 84, 84), _dy2(n, 84, 84)
    a = _run(cuda, fr, dy2)
    assert a[3] and FUSED in a[4], a[4]
    monkeypatch.setenv("AAA_VIS_BWD_FRAMES", "0")
    b = _run(cuda, fr, dy2)
    assert not b[3] and FUSED not in b[4], b[4]
    _same("CUs + 3: fused vs layered", a, b)
    assert N.pair_status(clear=True) == 0


def test_default_floor(cuda, monkeypatch):
    """With every default, fewer frames than CUs take the layered launches (measured faster there: DESIGN.md
    section 5, round 13); test_more_frames_than_cus_against_layered shows CUs + 3 fused by default."""
    monkeypatch.delenv("AAA_VBWD_MINF", raising=False)
    monkeypatch.delenv("AAA_VIS_BWD_FRAMES", raising=False)
    a = _run(cuda, _frames_u8(2, 84, 84), _dy2(2, 84, 84))
    assert not a[3] and FUSED not in a[4], a[4]


def test_dispatch_entry(cuda, monkeypatch):
    """Fused where the floor allows; AAA_VIS_BWD_FRAMES=0, fp32 frames and 210x160 take the layered launches."""
    monkeypatch.delenv("AAA_VIS_BWD_FRAMES", raising=False)
    monkeypatch.delenv("AAA_VIS_FRAMES", raising=False)
    fr, dy2 = _frames_u8(2, 84, 84), _dy2(2, 84, 84)
    a = _run(cuda, fr, dy2)
    assert a[3] and FUSED in a[4], a[4]
    monkeypatch.setenv("AAA_VIS_BWD_FRAMES", "0")
    b = _run(cuda, fr, dy2)
    assert not b[3] and FUSED not in b[4], b[4]
    _same("AAA_VIS_BWD_FRAMES=0", a, b)
    monkeypatch.delenv("AAA_VIS_BWD_FRAMES", raising=False)
    c = _run(cuda, fr.float(), dy2)
    assert not c[3] and FUSED not in c[4], c[4]
    _same("fp32 frames", a, c)
    big = _frames_u8(1, 210, 160)
    d = _run(cuda, big, _dy2(1, 210, 160))
    assert not d[3] and FUSED not in d[4], d[4]


def _learner(cuda, T, B):
    """One learner unroll + backward on uint8 frames -> (outputs, grads, the vision backward's variant)."""
    X = torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3))).to(cuda)
    Gl, Gv = (g.to(cuda) for g in _cot(T, B))
    ag = _agent(cuda)
    ag.reset()
    lg, vl, at = ag.unroll(X)
    N.timing_enable(True)
    try:
        ((lg * Gl).sum() + (vl * Gv).sum()).backward()
        torch.cuda.synchronize()
        var = N.timing_stats(N.TIMER_VISION_BWD)["variant"]
    finally:
        N.timing_enable(False)
    return (lg.detach().cpu(), vl.detach().cpu(), at.detach().cpu(), _grads(ag)), var


def test_end_to_end_vs_oracle(cuda, monkeypatch):
    monkeypatch.delenv("AAA_VIS_BWD_FRAMES", raising=False)
    out, var = _learner(cuda, 3, 2)
    assert FUSED in var, var
    _compare(out, _oracle(3, 2), RTOL, "fused fp32 encoder backward T=3 B=2: ")
    monkeypatch.setenv("AAA_VIS_BWD_FRAMES", "0")
    out0, var0 = _learner(cuda, 3, 2)
    assert FUSED not in var0, var0
    _compare(out0, _oracle(3, 2), RTOL, "layered fp32 encoder backward T=3 B=2: ")
    assert N.pair_status(clear=True) == 0


def test_packed_weights(cuda):
    """hi + mid + lo of the pre-split conv2 dgrad region (the last layout of the learner's packed buffer),
    un-permuted, is k_WdT2 within 2^-23, and k_WdT2 is the reference's weight by parity class."""
    runner = RT.UnrollRunner(1, 1, 84, 84, 4, 18, "fp32", cuda, frames_u8=True)
    flat = torch.cat([torch.from_numpy(np.asarray(v, np.float32)).reshape(-1) for v in PARAMS.values()]).to(cuda)
    packed = runner.new_packed()
    runner.pack(flat, packed)
    torch.cuda.synchronize()
    packed = packed.cpu()
    o_wdt2 = 32 * 256 * 4 + 64 * 512 * 4          # after k_Wp1 and k_Wp2 (fp32, 256-B aligned as they are)
    n = 4 * 32 * 256
    want = packed[o_wdt2:o_wdt2 + 4 * n].contiguous().view(torch.float32).reshape(128, 256)
    w2 = torch.as_tensor(np.ascontiguousarray(PARAMS[KEYS[2]])).float()   # (64, 32, kx, ky)
    for cls in range(4):   # W_c[ci][(ty*2+tx)*64 + co] = W2[co][ci][kx][ky], ky = py + 2(1-ty), kx = px + 2(1-tx)
        for t in range(4):
            ky, kx = (cls >> 1) + 2 * (1 - (t >> 1)), (cls & 1) + 2 * (1 - (t & 1))
            assert torch.equal(want[cls * 32:(cls + 1) * 32, t * 64:(t + 1) * 64], w2[:, :, kx, ky].t())
    raw = packed[-4 * 16 * 3 * 64 * 16:]
    parts = raw.contiguous().view(torch.bfloat16).reshape(4, 16, 3, 2, 32, 8)
    parts = parts.permute(2, 0, 4, 1, 3, 5).reshape(3, 128, 256).double()
    got = parts.sum(0)
    nz = want != 0
    rel = ((got - want.double()).abs()[nz] / want.double().abs()[nz]).max()
    print(f"conv2 dgrad classes: hi + mid + lo against k_WdT2, worst relative {float(rel):.3e}")
    assert float(rel) <= 2.0 ** -23, float(rel)
    assert torch.equal(got[~nz], torch.zeros_like(got[~nz]))
    assert bool((parts[2] != 0).any()), "the lo plane is all zero"
