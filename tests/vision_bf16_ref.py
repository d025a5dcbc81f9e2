"""fp64 references, bounds and cases shared by the bf16 vision-encoder tests
(test_vision_bf16_emulation.py on the CPU, test_gpu_vision_bf16.py on the GPU).

The bf16 encoder (VisionNetwork.vision_cnn, attention.py:155-170, on
X.transpose(1,3), :179) has no transcendental function and no fp16 store: every
operand of every GEMM is an exact bf16 value and every product is summed in
fp32, so there is ONE correct answer per element, ``bf16(fp64 result)``, and a
correct kernel misses it only where fp32 summation noise crosses a rounding
boundary.  The references are torch's fp64 convolutions in the reference's
orientation on

  * the weights rounded to bf16 by torch (round to nearest even), fp32 biases,
  * each kernel's OWN operand as the checker entry (aaa_vision_enc_*) hands it
    back: Y1 from the kernel's Xp, the conv2 output from the kernel's Y1, dY1 and
    gW2 from the dY2 given and the kernel's Y1, gW1 from the kernel's dY1 where
    the path that ran produces one.

Bounds (none of them comes from a device measurement):

  b. bf16 output of one fp32-accumulated GEMM (Y1, conv2 output, layered dY1):
     |k - y64| <= ulp_bf16(max(|y64|, |k|)) / 2 + K 2^-24 S per element, S the
     same conv on absolute values (+ |bias|), K the reduction length + 1 -- the
     worst-case fp32 summation error of any order (Higham, Accuracy and
     Stability of Numerical Algorithms, eq. 4.4).
  c. share of elements not bit-equal to bf16(y64): <= MISMATCH_CAP (1e-3) per
     tensor; two CPU fp32 orders stay <= MISMATCH_CPU (2.5e-4).  In a tensor
     too small to resolve the cap one element is allowed (share_ok).
  d. fp32 weight gradients with every operand known: norm-relative <= 1e-5 of
     fp64 (40 x the CPU fp32 reference's 2.5e-7).
  e. gW1 of the fused backward (its dY1 never leaves LDS): the reference rounds
     its own fp64 dY1 to bf16; the gate is 4 e_flip + 1e-5 with e_flip the change
     of the fp64 gW1 when dY1 is rounded from an fp32 evaluation of the dgrad
     instead -- the largest over five summation orders (fused_gw1_ref), computed
     per case from the reference alone.
  f. bias gradients: gb2 (column sum of dY2) 1e-5; gb1 1e-4 against the fp64 sum
     of dY1 BEFORE the bf16 rounding -- both backward paths sum the fp32
     accumulators in the dgrad's epilogue (csrc/vision_bwd.h "the bias sums from
     fp32"; rt_backward.hip conv2_dgrad).

Layouts.  The kernels keep images NHWC, (N, rows, cols, C); the reference's
(N, C, cols, rows) is ``t.permute(0, 3, 2, 1)`` either way (``to_ref``).
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from helpers import detinit

BF = torch.bfloat16
CNN = "vision.vision_cnn."
MISMATCH_CAP = 1e-3     # (c) on the device
MISMATCH_CPU = 2.5e-4   # (c) for the CPU fp32 orders: a factor 4 inside the cap
GATE_W = 1e-5           # (d)
GATE_B2, GATE_B1 = 1e-5, 1e-4   # (f)
K1, K2, KD = 256, 512, 256      # reduction length + 1 of conv1 (192 real taps, 256 with the 4th channel), conv2, dgrad

SOURCES = ("u8", "f32int", "f32s")   # uint8 frames, the same integers as fp32, fp32 x 0.37 (rounding visible)
FRAME_SCALE = 0.37

# (H, W): the frame-resident kernels' edges
G84, G80, G64, G20 = (84, 84), (80, 80), (64, 100), (20, 24)
RESIDENT_GEOS = (G84, G80, G64, G20)
RESIDENT_N = (1, 5)
# banded conv1 / conv2: (H, W, N, AAA_VIS_FRAMES)
BAND_CASES = ((168, 168, 2, "1"), (72, 168, 2, "1"), (40, 44, 3, "0"))
LAYERED_FWD = ((84, 84, 3), (80, 80, 3))
FUSED_GEOS = (G84, G80, G64)
FUSED_N = (1, 9, 17, 70)
# layered backward: (H, W, N, source).  32 / 64 frames: both weight gradients' K whole tiles (the rings);
# 80x80 x 3: 300 and 1083 pixel rows, neither a whole number of tiles; fp32 frames never take the fused kernel
LAYERED_BWD = ((84, 84, 32, "u8"), (80, 80, 64, "u8"), (64, 100, 32, "f32s"), (20, 24, 2, "u8"),
               (168, 168, 2, "f32s"), (80, 80, 3, "f32s"))
PIPES = ((1, 1), (2, 2), (1, 2), (2, 1))   # (AAA_CONV1_WGRAD_PIPE, AAA_CONV2_WGRAD_PIPE)


def geometry(H, W):
    H1, W1 = (H + 2 - 8) // 4 + 1, (W + 2 - 8) // 4 + 1
    return H1, W1, (H1 + 4 - 4) // 2 + 1, (W1 + 4 - 4) // 2 + 1


def cpu_cases():
    """Every (H, W, N, source) the GPU tests use (the CU-count case at the MI355X's 256 + 3)."""
    out = []
    for g in RESIDENT_GEOS:
        out += [(g[0], g[1], n, s) for n in RESIDENT_N for s in SOURCES]
    out.append((84, 84, 259, "u8"))
    out += [(H, W, n, s) for H, W, n, _ in BAND_CASES for s in ("u8", "f32s")]
    out += [(H, W, n, "u8") for H, W, n in LAYERED_FWD]
    out += [(g[0], g[1], n, "u8") for g in FUSED_GEOS for n in FUSED_N]
    out += list(LAYERED_BWD)
    return sorted(set(out))


# ------------------------------------------------------------------ inputs --
@functools.lru_cache(maxsize=None)
def weights():
    """(w1, b1, w2, b2) fp32 and the flat 39,008-float parameter vector."""
    P = detinit.deterministic_params(0, 18)
    t = [torch.from_numpy(np.ascontiguousarray(P[CNN + f"{i}.{n}"])) for i in (0, 1) for n in ("weight", "bias")]
    return t[0], t[1], t[2], t[3], torch.cat([x.reshape(-1) for x in t])


def frames(H, W, N, source, seed=1234):
    """(N, H, W, 3): uint8, or fp32 holding the same integers, or those x 0.37."""
    u8 = torch.from_numpy(detinit.frames_u8(seed + 7 * H + W, (N, H, W, 3)))
    if source == "u8":
        return u8
    x = u8.to(torch.float32)
    return x * FRAME_SCALE if source == "f32s" else x


def cot_dy2(N, P, seed=3):
    """dY2 (N, P, 64): uniform (-1, 1) rounded to bf16 on the host."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((N, P, 64), generator=g) * 2 - 1).to(BF)


def to_ref(t):
    return t.permute(0, 3, 2, 1)


# ------------------------------------------------------------------ bf16 ----
def ulp_bf16(v):
    """Spacing of bf16 numbers in the binade of |v| (fp64 tensor)."""
    a = v.abs().clamp_min(2.0 ** -126)
    _, e = torch.frexp(a)   # a = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), e - 8)


def bf16_rne(y64):
    """fp64 -> bf16, round to nearest even in ONE rounding (torch's double -> float -> bf16 rounds twice)."""
    c = y64.to(torch.float32).to(BF)
    ci = c.view(torch.int16).to(torch.int32)
    best, bi = c, ci
    bd = (c.double() - y64).abs()
    for d in (-1, 1):
        ni = ci + d
        cand = ni.to(torch.int16).view(BF)
        cd = (cand.double() - y64).abs()
        ok = torch.isfinite(cand.double()) & ((ci & 0x7FFF) + d >= 0)
        take = ok & ((cd < bd) | ((cd == bd) & ((ni & 1) == 0) & ((bi & 1) == 1)))
        best = torch.where(take, cand, best)
        bi = torch.where(take, ni, bi)
        bd = torch.where(take, cd, bd)
    return best


def trunc_bf16(y32):
    """fp32 -> bf16 by dropping the low 16 bits (the emulated cast fault)."""
    return (y32.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF)


def bound_b(k, y64, S, K):
    """(worst err / bound, worst err in bf16 ulps); bound (b) holds iff the first is <= 1.  NaN -> inf."""
    kd = k.double()
    u = ulp_bf16(torch.maximum(y64.abs(), kd.abs()))
    err = (kd - y64).abs()
    ratio = err / (0.5 * u + K * 2.0 ** -24 * S)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    eu = torch.where(torch.isfinite(err), err / u, torch.full_like(err, float("inf")))
    return float(ratio.max()), float(eu.max())


def mismatch_share(k, y64):
    """Share of elements of the bf16 tensor k that are not bf16(y64) (NaN counts)."""
    return float((k.float() != bf16_rne(y64).float()).double().mean())


def share_ok(k, y64, cap):
    """(c) -> (holds, share).  The cap limits a RATE, and a tensor of n elements shows only multiples of
    1 / n: below 1 / cap elements (the 20x24 frames: 576 to 3,200 per tensor) ONE element on a rounding
    boundary is already past it -- torch's own fp32 conv2 has one such element in the 2,880 of 5 frames
    of 20x24.  So the count allowed is cap * n rounded down, but never less than one element; wherever
    cap * n >= 1 that is the cap as stated.  Bound (b) still holds every element, that one included."""
    share = mismatch_share(k, y64)
    n = k.numel()
    return round(share * n) <= max(1, int(cap * n)), share


def rel(a, b):
    a, b = a.double(), b.double()
    nb = float(b.norm())
    d = float((a - b).norm())
    if not np.isfinite(d):
        return float("inf")
    return d / nb if nb > 0 else d


# -------------------------------------------------------------- references --
def xp_expected(fr):
    """(a): the bordered RGBx image of the frames, bf16(frame) inside, zero border and channel 3."""
    N, H, W, _ = fr.shape
    xp = torch.zeros((N, H + 2, W + 2, 4), dtype=BF)
    xp[:, 1:-1, 1:-1, :3] = fr.to(torch.float32).to(BF)
    return xp


def _x_ref(xp):
    """Conv1's operand from a bordered image (N, H+2, W+2, 4): its interior, reference orientation, fp64."""
    return to_ref(xp[:, 1:-1, 1:-1, :3].double()).contiguous()


def conv1_ref(xp, dtype=torch.float64):
    """-> (y1, S) in the kernels' layout (N, H1, W1, 32), evaluated in ``dtype`` on the bf16 weights."""
    w1, b1, _, _, _ = weights()
    x, w = _x_ref(xp).to(dtype), w1.to(BF).to(dtype)
    y = F.conv2d(x, w, b1.to(dtype), stride=4, padding=1)
    S = F.conv2d(x.abs(), w.abs(), b1.to(dtype).abs(), stride=4, padding=1)
    return to_ref(y).contiguous(), to_ref(S).contiguous()


def conv2_ref(y1, dtype=torch.float64):
    """y1 (N, H1, W1, 32) bf16 -> (x2, S) (N, h, w, 64)."""
    _, _, w2, b2, _ = weights()
    x, w = to_ref(y1.to(dtype)).contiguous(), w2.to(BF).to(dtype)
    y = F.conv2d(x, w, b2.to(dtype), stride=2, padding=2)
    S = F.conv2d(x.abs(), w.abs(), b2.to(dtype).abs(), stride=2, padding=2)
    return to_ref(y).contiguous(), to_ref(S).contiguous()


def dgrad_ref(dy2, H1, W1, dtype=torch.float64):
    """dy2 (N, h, w, 64) bf16 -> (dy1, S) (N, H1, W1, 32)."""
    _, _, w2, _, _ = weights()
    g, w = to_ref(dy2.to(dtype)).contiguous(), w2.to(BF).to(dtype)
    shp = (dy2.shape[0], 32, W1, H1)
    d = conv2d_input(shp, w, g, stride=2, padding=2)
    S = conv2d_input(shp, w.abs(), g.abs(), stride=2, padding=2)
    return to_ref(d).contiguous(), to_ref(S).contiguous()


def gw2_ref(y1, dy2, dtype=torch.float64):
    """conv2's weight gradient (64, 32, 4, 4) from y1 (N, H1, W1, 32) and dy2 (N, h, w, 64), both bf16."""
    return conv2d_weight(to_ref(y1.to(dtype)).contiguous(), (64, 32, 4, 4), to_ref(dy2.to(dtype)).contiguous(),
                         stride=2, padding=2)


def gw1_ref(xp, dy1, dtype=torch.float64):
    """conv1's weight gradient (32, 3, 8, 8) from the bordered image and dy1 (N, H1, W1, 32) bf16."""
    return conv2d_weight(_x_ref(xp).to(dtype), (32, 3, 8, 8), to_ref(dy1.to(dtype)).contiguous(), stride=4, padding=1)


def split_grads(g):
    """flat (39,008) -> (gW1 (32,3,8,8), gb1 (32), gW2 (64,32,4,4), gb2 (64))."""
    g = g.detach().cpu().double()
    return (g[:6144].reshape(32, 3, 8, 8), g[6144:6176], g[6176:6176 + 32768].reshape(64, 32, 4, 4),
            g[6176 + 32768:])


def fused_gw1_ref(xp, dy2, H1, W1):
    """(e): (gW1 from the reference's own bf16(dY1_fp64), e_flip).

    e_flip is the LARGEST change of the fp64 gW1 over dgrad_f32_all's five fp32 evaluations of the
    dgrad.  One evaluation is not a yardstick: a handful of dY1 elements sit on a rounding boundary
    (8 to 12 of 115,200 at 9 frames of 84x84), which of them flip depends on the summation order, and
    one large element decides the figure -- torch's own order gives 3.5e-7 there, the four others 2.1 to
    2.3e-5 ("bf16 vision encoder: accuracy")."""
    d64, _ = dgrad_ref(dy2, H1, W1)
    g = gw1_ref(xp, bf16_rne(d64))
    return g, max(rel(gw1_ref(xp, d.to(BF)), g) for d in dgrad_f32_all(dy2, H1, W1))


# --------------------------------------------------- CPU fp32, two orders ---
def conv1_f32_orders(xp):
    """conv1 in fp32: torch's order, and the three input channels summed one by one (2, 0, 1)."""
    w1, b1, _, _, _ = weights()
    x, w = _x_ref(xp).float(), w1.to(BF).float()
    a = F.conv2d(x, w, b1, stride=4, padding=1)
    b = sum(F.conv2d(x[:, c:c + 1], w[:, c:c + 1], None, stride=4, padding=1) for c in (2, 0, 1))
    return to_ref(a).contiguous(), to_ref(b + b1[None, :, None, None]).contiguous()


def conv2_f32_orders(y1, pad_fault=False):
    """conv2 in fp32: torch's order, and four 8-channel groups (3, 1, 0, 2).  pad_fault: the border row
    next to the map's first row holds a copy of that row instead of zeros (the emulated border fault)."""
    _, _, w2, b2, _ = weights()
    x, w = to_ref(y1.float()).contiguous(), w2.to(BF).float()
    xp = F.pad(x, (2, 2, 2, 2))
    if pad_fault:
        xp[:, :, :, 1] = xp[:, :, :, 2]
    a = F.conv2d(xp, w, b2, stride=2)
    b = sum(F.conv2d(xp[:, 8 * g:8 * g + 8], w[:, 8 * g:8 * g + 8], None, stride=2) for g in (3, 1, 0, 2))
    return to_ref(a).contiguous(), to_ref(b + b2[None, :, None, None]).contiguous()


def dgrad_f32_orders(dy2, H1, W1):
    _, _, w2, _, _ = weights()
    g, w = to_ref(dy2.float()).contiguous(), w2.to(BF).float()
    shp = (dy2.shape[0], 32, W1, H1)
    a = conv2d_input(shp, w, g, stride=2, padding=2)
    b = sum(conv2d_input(shp, w[16 * q:16 * q + 16], g[:, 16 * q:16 * q + 16], stride=2, padding=2)
            for q in (2, 0, 3, 1))
    return to_ref(a).contiguous(), to_ref(b).contiguous()


def dgrad_f32_all(dy2, H1, W1):
    """Five fp32 evaluations of the dgrad: torch's, three orders of four 16-channel groups, and the
    fused kernel's loop order (taps outside, 16-channel k steps inside, one running fp32 sum)."""
    _, _, w2, _, _ = weights()
    g, w = to_ref(dy2.float()).contiguous(), w2.to(BF).float()
    shp = (dy2.shape[0], 32, W1, H1)

    def part(wt, q):
        return conv2d_input(shp, wt[16 * q:16 * q + 16], g[:, 16 * q:16 * q + 16], stride=2, padding=2)
    out = [conv2d_input(shp, w, g, stride=2, padding=2)]
    out += [sum(part(w, q) for q in perm) for perm in ((2, 0, 3, 1), (0, 1, 2, 3), (3, 2, 1, 0))]
    acc = torch.zeros(shp)
    for ky in range(4):
        for kx in range(4):
            wt = torch.zeros_like(w)
            wt[:, :, ky, kx] = w[:, :, ky, kx]
            for q in range(4):
                acc = acc + part(wt, q)
    out.append(acc)
    return [to_ref(o).contiguous() for o in out]


def per_frame_sum(fn, N):
    """A weight gradient accumulated frame by frame in fp32 (the second order)."""
    acc = None
    for n in range(N - 1, -1, -1):
        t = fn(n)
        acc = t if acc is None else acc + t
    return acc
