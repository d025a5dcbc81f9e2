"""The learner's bf16 vision-encoder kernels, each against fp64 on its OWN operands
(bounds, references and cases: tests/vision_bf16_ref.py; CPU evidence that the gates
hold for correct arithmetic and fail for three kernel faults:
tests/test_vision_bf16_emulation.py).

The kernels run through the checker entries aaa_vision_enc_fwd / _bwd (runtime.py
EncRunner), which call the learner's own dispatch -- vision_fwd<bf16, bf16> and the
VISION phase of the backward -- and hand back the raw bf16 products:

  k_vision_fwd            frame-resident conv1 + conv2 (C3 / C4)
  k_vision_conv1_band,
  k_vision_conv2_band     banded conv1 / conv2 for frames too large for it (C5)
  layered forward         frames_rgbx + the im2col rings writing bf16
  k_vision_bwd_frames     fused conv2 wgrad + dgrad + conv1 wgrad
  layered backward        halo-staged conv2 dgrad, conv2 / conv1 weight-gradient rings

Every test asserts from the library's launch record (aaa_timing_stats) that the kernel
it names is the one that ran, prints its figures before it asserts, and ends with no
partner timeout reported.  Reference: attention.py:155-170 on X.transpose(1,3) (:179)
and its autograd backward."""
import pytest
import torch

import attention
import vision_bf16_ref as R

pytestmark = pytest.mark.gpu
N = attention._pkg._native
RT = attention._pkg.runtime
BF = torch.bfloat16
ENV = ("AAA_VIS_FRAMES", "AAA_VIS_BAND", "AAA_VIS_BAND2", "AAA_VIS_BWD_FRAMES", "AAA_VBWD_MINF",
       "AAA_CONV1_WGRAD_PIPE", "AAA_CONV2_WGRAD_PIPE")


def _setenv(monkeypatch, **env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _timed(kind, fn):
    N.timing_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        st = N.timing_stats(kind)
    finally:
        N.timing_enable(False)
    return out, st


class Run:
    """One forward through aaa_vision_enc_fwd: the inputs, the kernels' products (host copies), the variant."""

    def __init__(self, cuda, H, W, n, src, out_ld=192):
        self.H, self.W, self.n, self.src = H, W, n, src
        self.H1, self.W1, self.h, self.w = R.geometry(H, W)
        self.fr = R.frames(H, W, n, src)
        self.enc = RT.EncRunner(n, H, W, out_ld=out_ld, frames_u8=src == "u8", device=cuda)
        self.flat = R.weights()[4].to(cuda)
        self.packed = self.enc.pack(self.flat)
        self.frd = self.fr.to(cuda)
        (self.xp_d, self.y1_d, self.out_d), st = _timed(
            N.TIMER_VISION_FWD, lambda: self.enc.forward(self.flat, self.packed, self.frd))
        assert st["launches"] == 1, st
        self.variant = st["variant"]
        self.xp, self.y1, self.out = self.xp_d.cpu(), self.y1_d.cpu(), self.out_d.cpu()

    def backward(self, dy2):
        (g, dy1, fused), st = _timed(
            N.TIMER_VISION_BWD, lambda: self.enc.backward(self.packed, self.frd, dy2, self.y1_d, self.xp_d))
        assert st["launches"] == 1, st
        assert ("k_vision_bwd_frames" in st["variant"]) == fused, (st, fused)
        return R.split_grads(g), (None if dy1 is None else dy1.cpu()), fused


def _bits(t):
    return t.contiguous().view(torch.int16)


def _tensor_bounds(what, k, y64, S, K):
    """(b) and (c) for one bf16 product."""
    ratio, ulps = R.bound_b(k, y64, S, K)
    ok, share = R.share_ok(k, y64, R.MISMATCH_CAP)
    print(f"{what}: {k.numel()} elements, mismatch share {share:.2e}, worst {ulps:.4f} ulp, err / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, "bound (b)", ratio, ulps)
    assert ok, (what, "share (c)", share)


def _check_forward(run, what, xp_rows=None):
    """(a), (b), (c), (g) on one forward's products.  xp_rows: the bordered rows the path writes
    (None: all H + 2; the banded conv1 writes the 4 H1 + 4 that conv1 reads)."""
    exp = R.xp_expected(run.fr)
    rows = run.H + 2 if xp_rows is None else xp_rows
    assert torch.equal(_bits(run.xp[:, :rows]), _bits(exp[:, :rows])), f"{what}: Xp is not bf16(frame), zero-bordered"
    xk = run.xp.clone()
    xk[:, rows:] = 0   # (never read by conv1: its last window ends at row 4 H1 + 3)
    y64, S1 = R.conv1_ref(xk)
    _tensor_bounds(f"{what} Y1", run.y1, y64, S1, R.K1)
    x64, S2 = R.conv2_ref(run.y1)
    x2 = run.out[:, :, :64].reshape(run.n, run.h, run.w, 64)
    _tensor_bounds(f"{what} conv2 out", x2, x64, S2, R.K2)
    if run.out.shape[2] > 64:   # the h half of the learner's [x | h] rows
        assert bool((_bits(run.out[:, :, 64:]) == RT.EncRunner.SENTINEL).all()), f"{what}: columns 64.. were written"
    return xk


def _check_grads(what, grads, run, xk, dy2, gate1, g1_ref, d64):
    """(d) / (e) and (f).  dy2 (N, P, 64); g1_ref: conv1's weight-gradient reference, at gate1."""
    gW1, gb1, gW2, gb2 = grads
    dy2i = dy2.reshape(run.n, run.h, run.w, 64)
    e2 = R.rel(gW2, R.gw2_ref(run.y1, dy2i))
    e1 = R.rel(gW1, g1_ref)
    eb2 = R.rel(gb2, dy2.double().sum((0, 1)))
    eb1 = R.rel(gb1, d64.sum((0, 1, 2)))
    print(f"{what}: gW2 {e2:.2e} / {R.GATE_W:.0e}, gW1 {e1:.2e} / {gate1:.2e}, gb2 {eb2:.2e}, gb1 {eb1:.2e}")
    assert e2 <= R.GATE_W, (what, "gW2", e2)
    assert e1 <= gate1, (what, "gW1", e1, gate1)
    assert eb2 <= R.GATE_B2 and eb1 <= R.GATE_B1, (what, eb2, eb1)


def _done():
    assert N.pair_status(clear=True) == 0


# ---------------------------------------------------------------- forward ---
@pytest.mark.parametrize("src", R.SOURCES)
@pytest.mark.parametrize("n", R.RESIDENT_N)
@pytest.mark.parametrize("H,W", R.RESIDENT_GEOS)
def test_frame_resident_forward(cuda, monkeypatch, H, W, n, src):
    """k_vision_fwd at the workload's geometry, an odd conv1 map with a 9-pixel last column block
    (80x80), a non-square frame (64x100: orientation, W1 != H1) and maps under one 32-pixel block
    (20x24); the learner's row pitch 192 and a dense 64."""
    _setenv(monkeypatch)
    for out_ld in (192, 64):
        run = Run(cuda, H, W, n, src, out_ld)
        assert "k_vision_fwd" in run.variant, run.variant
        _check_forward(run, f"resident {H}x{W} N={n} {src} ld={out_ld}")
    _done()


def test_frame_resident_forward_second_pass(cuda, monkeypatch):
    """CUs + 3 frames of 84x84: every persistent workgroup prefetches a second frame under the first
    one's convs, three of them go on to it and the others do not."""
    _setenv(monkeypatch)
    n = torch.cuda.get_device_properties(cuda).multi_processor_count + 3
    run = Run(cuda, 84, 84, n, "u8")
    assert "k_vision_fwd" in run.variant, run.variant
    _check_forward(run, f"resident 84x84 N={n} u8")
    _done()


@pytest.mark.parametrize("src", ("u8", "f32s"))
@pytest.mark.parametrize("H,W,n,frames_env", R.BAND_CASES)
def test_banded_forward(cuda, monkeypatch, H, W, n, frames_env, src):
    """k_vision_conv1_band + k_vision_conv2_band: 168x168 (conv1 bands 8,8,8,8,8,1; conv2 8,8,5), 72x168
    (8,8,1 and 8,1; too large for the frame-resident kernel, so the banded path by itself) and 40x44
    with the frame-resident kernel switched off (8,1; one conv2 band).  Xp must be complete over the
    rows conv1 reads: every band its own, the last one the 4 below."""
    _setenv(monkeypatch, AAA_VIS_FRAMES=frames_env)
    run = Run(cuda, H, W, n, src)
    assert "k_vision_conv1_band" in run.variant and "k_vision_conv2_band" in run.variant, run.variant
    _check_forward(run, f"banded {H}x{W} N={n} {src}", xp_rows=4 * run.H1 + 4)
    _done()


@pytest.mark.parametrize("H,W,n", R.LAYERED_FWD)
def test_layered_forward(cuda, monkeypatch, H, W, n):
    """frames_rgbx and the bf16 im2col conv1 ring / conv2 GEMM writing bf16 (AAA_VIS_FRAMES=0,
    AAA_VIS_BAND=0) -- not the fp32 output of the aaa_vision_cnn_fwd path."""
    _setenv(monkeypatch, AAA_VIS_FRAMES=0, AAA_VIS_BAND=0)
    run = Run(cuda, H, W, n, "u8")
    assert "layered" in run.variant and "k_vision" not in run.variant, run.variant
    _check_forward(run, f"layered {H}x{W} N={n}")
    _done()


# --------------------------------------------------------------- backward ---
def _fused_case(cuda, monkeypatch, H, W, n, dy2, what):
    _setenv(monkeypatch)
    run = Run(cuda, H, W, n, "u8")
    assert "k_vision_fwd" in run.variant, run.variant
    xk = run.xp
    grads, dy1, fused = run.backward(dy2)
    assert fused and dy1 is None, "the fused backward did not run"
    d64, _ = R.dgrad_ref(dy2.reshape(n, run.h, run.w, 64), run.H1, run.W1)
    g1_ref, e_flip = R.fused_gw1_ref(xk, dy2.reshape(n, run.h, run.w, 64), run.H1, run.W1)
    gate = 4 * e_flip + 1e-5
    _check_grads(f"fused {what}", grads, run, xk, dy2, gate, g1_ref, d64)
    _setenv(monkeypatch, AAA_VIS_BWD_FRAMES=0)
    lay, dy1l, fused_l = run.backward(dy2)
    assert not fused_l and dy1l is not None
    e = R.rel(grads[0], lay[0])
    print(f"fused {what}: gW1 fused vs layered {e:.2e} / {gate:.2e} (e_flip {e_flip:.2e})")
    assert e <= gate, (what, e, gate)
    _done()
    return grads, run


@pytest.mark.parametrize("n", R.FUSED_N)
@pytest.mark.parametrize("H,W", R.FUSED_GEOS)
def test_fused_backward(cuda, monkeypatch, H, W, n):
    """k_vision_bwd_frames: one workgroup and no loop (1 frame), one workgroup looping over nine with the
    next frame's DMA in flight, two workgroups of unequal share (17) and eight (70).  gW2 against fp64
    on the kernel's own Y1 (d); gW1 -- its dY1 never leaves LDS -- against the reference's own rounded
    dY1 and against the layered launches, both at 4 e_flip + 1e-5 (e); the bias gradients (f): gb1 is
    the sum of the dgrad's fp32 accumulators, before their rounding to bf16."""
    P = R.geometry(H, W)[2] * R.geometry(H, W)[3]
    _fused_case(cuda, monkeypatch, H, W, n, R.cot_dy2(n, P), f"{H}x{W} N={n}")


def test_fused_backward_single_pixel(cuda, monkeypatch):
    """dY2 non-zero in the last frame's last grid pixel only: conv2's weight gradient is one outer
    product of bf16 values, exact in fp32 -- every other frame and pixel must contribute nothing."""
    H, W, n = 84, 84, 9
    P = 121
    dy2 = torch.zeros((n, P, 64), dtype=BF)
    dy2[-1, -1] = R.cot_dy2(1, 1)[0, 0]
    grads, run = _fused_case(cuda, monkeypatch, H, W, n, dy2, f"{H}x{W} N={n} single pixel")
    assert torch.equal(grads[2], R.gw2_ref(run.y1, dy2.reshape(n, 11, 11, 64))), "gW2 is not the exact outer product"


_LAYERED = {}


def _layered_inputs(cuda, H, W, n, src):
    """The forward's products and the references that do not depend on the weight-gradient kernels, once
    per case (the forward is deterministic; the four pipe settings share them)."""
    key = (H, W, n, src)
    if key not in _LAYERED:
        run = Run(cuda, H, W, n, src)
        dy2 = R.cot_dy2(n, run.h * run.w)
        d64, SD = R.dgrad_ref(dy2.reshape(n, run.h, run.w, 64), run.H1, run.W1)
        xk = run.xp.clone()
        xk[:, 4 * run.H1 + 4:] = 0   # (rows the banded conv1 leaves alone; no kernel reads them)
        _LAYERED.clear()              # one case's buffers at a time
        _LAYERED[key] = (run, dy2, d64, SD, xk)
    return _LAYERED[key]


@pytest.mark.parametrize("p1,p2", R.PIPES)
@pytest.mark.parametrize("H,W,n,src", R.LAYERED_BWD)
def test_layered_backward(cuda, monkeypatch, H, W, n, src, p1, p2):
    """The three layered launches (AAA_VIS_BWD_FRAMES=0, or fp32 frames, which never take the fused
    kernel) with both weight-gradient rings as pipe (1) and read-ahead (2): the halo-staged conv2
    dgrad's bf16 dY1 elementwise (b), (c) -- the odd maps of 80x80 (19x19: two parity classes are a
    row or a column short) and 64x100 included, last row and column checked on their own -- and both
    weight gradients against fp64 on the operands the kernels read, dY1 included (d).  32 / 64 frames
    make both K whole tiles; 3 frames of 80x80 (300 and 1083 pixel rows) make neither."""
    _setenv(monkeypatch)
    run, dy2, d64, SD, xk = _layered_inputs(cuda, H, W, n, src)
    _setenv(monkeypatch, AAA_VIS_BWD_FRAMES=0, AAA_CONV1_WGRAD_PIPE=p1, AAA_CONV2_WGRAD_PIPE=p2)
    grads, dy1, fused = run.backward(dy2)
    assert not fused and dy1 is not None, "the layered backward did not run"
    what = f"layered {H}x{W} N={n} {src} pipes {p1},{p2}"
    _tensor_bounds(f"{what} dY1", dy1, d64, SD, R.KD)
    for name, sl in (("last row", (slice(None), -1)), ("last column", (slice(None), slice(None), -1))):
        ratio, ulps = R.bound_b(dy1[sl], d64[sl], SD[sl], R.KD)
        assert ratio <= 1.0, (what, name, ratio, ulps)
    _check_grads(what, grads, run, xk, dy2, R.GATE_W, R.gw1_ref(xk, dy1), d64)
    _done()
