"""fp64 references, bounds, cases and the CPU stand-in shared by the bf16 ConvLSTM
tests (test_convlstm_bf16_emulation.py on the CPU, test_gpu_convlstm_bf16.py on
the GPU).

The bf16 recurrence (ConvLSTMCell.forward, attention.py:110-126, over T steps,
and its autograd backward) multiplies bf16 operands and sums in fp32.  Every
step is checked ALONE, in torch fp64, on

  * the weights rounded to bf16 by torch (round to nearest even), fp32 biases,
  * the kernel's OWN stored operands of that step, read back from the workspace
    (include/aaa.h AAA_BF16_WS_*): x_t, h_{t-1} (bf16), c_{t-1} (fp32), the gate
    activations (fp16), dO_t (fp32), dZ_{t+1} (bf16),
  * never another kernel's output and never the reference's own previous step --
    so nothing compounds, and bf16 / fp16 stores have ONE correct answer each.

What the kernels compute (csrc/recur.h, recur_bwd.h, epilogues.h), restated:
  forward   Z_t = Wx * x_t + b + Wh * h_{t-1};  i, f, o = sigma(Z), g = tanh(Z);
            c_t = f c_{t-1} + i g (fp32 store);  h_t = o tanh(c_t) (bf16 store);
            gates (i, f, g, o) stored fp16.
  BPTT      dh_t = dO_t + Wh^T * dZ_{t+1}   (dh_{T-1} = dO_{T-1} + dhT)
            tc = tanh(cc);  dcc = dc + dh o (1 - tc^2);  dZ_t = (dcc g (1-i) i,
            dcc c_{t-1} (1-f) f, dcc i (1 - g^2), dh tc (1-o) o);  dc <- dcc f
            with i, f, g, o the STORED fp16 gates.  cc is
              - the stored c_t in the per-step chain (epilogues.h EpiConvLstmBwd
                ``ccur``, rt_backward.hip bptt_step), mode "stored";
              - f c_{t-1} + i g recomputed from the fp16 gates in the frame-resident,
                paired and band kernels (recur_bwd.h gate_bwd_fast's 4th argument,
                lines 403 / 452 / 921: they never load c_t), mode "recomputed".
            dx_t = Wx^T * dZ_t (bf16 store);  dh0 = Wh^T * dZ_0, dc0 (fp32);
            gWx, gWh = sum_t dZ_t (x) [x_t | h_{t-1}] on the stored bf16 operands.
  bias sums gate bias: the frame-resident kernels sum the fp32 dz BEFORE the bf16
            rounding (recur_bwd.h:406 / 455 / 924 ``bs[..] += di``, stored per
            (step, frame) at :509 and column-summed, rt_backward.hip:1146); the
            per-step chain does the same on its ring tiles (EpiConvLstmBwd::Acc,
            epilogues.h:399) and sums the ROUNDED dZ otherwise (colsum<T> of dZ,
            rt_backward.hip:1150).  Every tile that serves fp16 gates is a ring
            tile (step_tiles.h BpttTiles, kG16), so with fp16 gates the sum is
            the fp32 one; only a run with fp32 gate storage (AAA_GATES_F16=0) is
            held to the nearer of the two references ("either").
            conv2 bias (dx's column sum): fp32 before the rounding on both paths
            (recur_bwd.h:707 ``xbs[..] += v[e]``; rt_backward.hip:841
            EpiStoreBiasT "summed from the fp32 values").
            So the references are the fp64 sums of the UNROUNDED fp64 dZ / dx.

Bounds.  u = 2^-24.  None comes from a device measurement.

  A_ACT  sigm_fast(z) = rcp(1 + exp2(-z * log2e)) (recur.h:82): the argument
         a = fl(z * fl(log2e)) carries a relative error <= 2u, which exp2 turns
         into a relative error |z| 2u of e = exp(-z); v_exp_f32 adds one ulp
         (<= 2u relative), the addition u and v_rcp_f32 one ulp (2u) relative to
         the result.  d sigma / de = -sigma^2, so
           |err| <= sigma (1 - sigma) (2u |z| + 2u) + sigma 3u
                 <= 2u (0.2239 + 0.25) + 3u < 4u          (max_z sigma(1-sigma)|z| = 0.2239)
         A_SIG = 4u = 2.4e-7.  tanh_fast(x) = 2 sigm_fast(2x) - 1 (2x exact):
         2 A_SIG + u for the subtraction: A_TANH = 9u = 5.4e-7.  The per-step
         kernels' expf / tanhf (sigm_acc, common.h:42) are within 2 ulp: inside both.
  dZ     = K u S, the worst-case fp32 summation error of any order (Higham,
         Accuracy and Stability of Numerical Algorithms, eq. 4.4): S the same
         convolutions on absolute values (+ |b|), K the reduction length + 1:
         KZ = 1729 for Z, KD = 4609 for the two dgrads.
         d_sigma = dZ / 4 + A_SIG,  d_tanh = dZ + A_TANH  (|sigma'| <= 1/4, |tanh'| <= 1).

  (a) fp32-stored results of known operands -- c_t, dh0, dc0, gWx, gWh, and the
      gate bias where it sums the stored dZ: norm-relative <= GATE_A = 1e-5 of
      fp64, the project's gate for this situation (vision_bf16_ref.GATE_W).  Plain
      float32 sits at 1e-7 (c_t), <= 3.2e-7 (dh0, dc0) and <= 1.1e-6 (gWx, gWh, the
      K-loop-edge cases) on the CPU: test_convlstm_bf16_emulation.py holds the
      stand-ins to GATE_A / 4.  Bias sums the kernel takes from unrounded fp32
      values: the reference's unrounded fp64 sum and GATE_BSUM = 1e-4 (GATE_B1).
  (b) c_t per element: |c - c64| <= |c_{t-1}| d_f + |g| d_i + |i| d_g
      + 3u (|f c_{t-1}| + |i g|)   (the last term: the two products and the sum).
  (c) rounded stores (fp16 gates, bf16 h_t, dZ_t, dx_t):
      |k - y64| <= ulp_store(max(|y64|, |k|)) / 2 + d_y, d_y the first-order
      propagation of dZ, A_ACT and (b) through the formula of y (fwd_step /
      bwd_step below write each out), every fp32 operation adding u |result|.
  (d) share of elements not bit-equal to the correctly rounded fp64 value:
      <= CAP_DEV = 2e-3 per tensor on the device, <= CAP_CPU = 1e-3 for the CPU
      stand-ins; one element is allowed in a tensor too small to resolve the cap
      (vision_bf16_ref.share_ok).

The cell entry (aaa_convlstm_cell_fwd / _bwd) keeps its gates and dZ to itself: cell_ref below.

What rejects which emulated defect (test_convlstm_bf16_emulation.py): DEFECTS below.
(b) alone rejects none of them that (a) / (c) / (d) do not: its K u S term is three
orders above fp32's real noise; it is the per-element backstop of (a)'s norm.

Layouts.  The kernels keep images pixel-major, channel fastest: (B*h*w, C) rows;
the references run in the reference implementation's orientation (B, C, w, h)
(f32_split_ref.to_ref / from_ref).  Channel-quad-major slices (include/aaa.h) are
de-permuted on the host by ``from_cqm4`` / ``from_cqmg`` from the header's maps.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

import f32_split_ref as R
import vision_bf16_ref as V
from helpers import detinit
from oracle import ref_cpu

BF, F16 = torch.bfloat16, torch.float16
U = 2.0 ** -24
A_SIG, A_TANH = 4 * U, 9 * U
KZ, KD = 1729, 4609
GATE_A, GATE_BSUM = 1e-5, 1e-4
CAP_DEV, CAP_CPU = 2e-3, 1e-3
LOG2E = 1.4426950408889634

# (T, B, H, W, carried state).  84x84: 11x11 grid, P = 121, seven padding columns of 128; B = 9: a ragged second
# XCD group of eight frames; 64x64: P = 64; carried state: non-zero h0 / c0 and dhT / dcT at dO's scale;
# 64x100: an 8x13 grid (H != W, P = 104, inside rec_fits: 104 <= 128, 10 x 15 <= 169)
UNROLL_CASES = [(3, 2, 84, 84, False), (2, 9, 84, 84, False), (4, 3, 64, 64, False), (3, 2, 84, 84, True),
                (2, 2, 64, 100, False)]
# 168x168: 21x21 grid, bands of 5, 5, 5, 6 rows; B = 5: padding workgroups of the last XCD column
BAND_CASES = [(2, 2, 168, 168, False), (3, 5, 168, 168, True)]
WGRAD_EDGE_CASES = R.WGRAD_EDGE_CASES
CELL_CASES = R.CELL_CASES
# The frames are detinit's integers x 1/16 (exact).  Raw 0..255 frames drive the gate pre-activations to a standard
# deviation of 31: nearly every gate saturates, most |c_t| and |h_t| fall below 1e-5, where tanh_fast's ABSOLUTE
# accuracy (A_TANH) is a large relative error and a bf16 store has no single fp32-reachable answer -- and where a
# wrong operand hides behind a saturated sigma.  At 1/16 the pre-activations have a standard deviation of 1.9
# (|Z| <= 8.3): every gate is live and (d) resolves.
FRAME_SCALE = 1.0 / 16

# emulated defect -> the (bound, observable) that must reject it
DEFECTS = {
    "trunc_h": ("d", "h"),            # h_t stored by truncation
    "trunc_dz": ("d", "dz"),          # dZ_t stored by truncation
    "border_taps": ("a", "c"),        # the three taps of one border column of the h image dropped
    "stale_row": ("a", "c"),          # one band-boundary row of h_{t-1} taken from h_{t-2}
    "splitk_bf16": ("a", "gWh"),      # split-K partials of the weight gradient rounded to bf16 before the sum
    "sigma_1e-5": ("d", "gates"),     # sigma off by 1e-5 absolute
    "gates_fp32_bwd": ("d", "dz"),    # the BPTT reads unrounded gates where the kernel stores fp16
}


def case_id(c):
    return "T{}B{}_{}x{}{}".format(*c[:4], "_state" if c[4] else "")


# ------------------------------------------------------- channel-quad-major --
def cqm4_index(P):
    """(P, 128) element offsets of (pixel, channel) in a channel-quad-major 128-channel slice (include/aaa.h)."""
    pp, ch = torch.arange(P)[:, None], torch.arange(128)[None, :]
    return ((ch >> 2) * P + pp) * 4 + (ch & 3)


def cqmg_index(P):
    """(P, 512) element offsets of (pixel, column 4*ch + gate) in a channel-quad-major gate slice."""
    pp, col = torch.arange(P)[:, None], torch.arange(512)[None, :]
    ch, gate = col >> 2, col & 3
    return ((ch >> 2) * P + pp) * 16 + (ch & 3) * 4 + gate


def _from_cqm(buf, P, idx):
    """buf (..., B*P, C) whose (frame) slices of P*C elements are permuted by idx -> row-major (..., B*P, C)."""
    lead, (M, C) = buf.shape[:-2], buf.shape[-2:]
    assert M % P == 0
    fr = buf.reshape(*lead, M // P, P * C)
    return fr[..., idx.reshape(-1)].reshape(*lead, M, C)


def from_cqm4(buf, P):
    return _from_cqm(buf, P, cqm4_index(P))


def from_cqmg(buf, P):
    return _from_cqm(buf, P, cqmg_index(P))


# ---------------------------------------------------------------- rounding --
def _mant(dtype):
    return {BF: 8, F16: 11, torch.float32: 24}[dtype]


def ulp_store(v, dtype):
    """Spacing of ``dtype`` numbers in the binade of |v| (fp64 tensor); fp16's subnormal spacing below 2^-14."""
    a = v.abs().clamp_min(2.0 ** -126)
    _, e = torch.frexp(a)
    u = torch.ldexp(torch.ones_like(a), e - _mant(dtype))
    return u.clamp_min(2.0 ** -24) if dtype == F16 else u


def rne(y64, dtype):
    """fp64 -> dtype, round to nearest even in ONE rounding (torch's double -> float -> dtype rounds twice)."""
    if dtype == torch.float32:
        return y64.to(torch.float32)
    c = y64.to(torch.float32).to(dtype)
    ci = c.view(torch.int16).to(torch.int32)
    best, bi = c, ci
    bd = (c.double() - y64).abs()
    for d in (-1, 1):
        ni = ci + d
        cand = ni.to(torch.int16).view(dtype)
        cd = (cand.double() - y64).abs()
        ok = torch.isfinite(cand.double()) & ((ci & 0x7FFF) + d >= 0)
        take = ok & ((cd < bd) | ((cd == bd) & ((ni & 1) == 0) & ((bi & 1) == 1)))
        best = torch.where(take, cand, best)
        bi = torch.where(take, ni, bi)
        bd = torch.where(take, cd, bd)
    return best


def share(k, y64):
    """(holds at cap?, share) helper: share of elements of the stored tensor k that are not rne(y64) (NaN counts)."""
    return float((k.double() != rne(y64, k.dtype).double()).double().mean())


def share_ok(k, y64, cap):
    """(d) with vision_bf16_ref.share_ok's rule: cap * n elements rounded down, never less than one."""
    s = share(k, y64)
    n = k.numel()
    return round(s * n) <= max(1, int(cap * n)), s


def bound_c(k, y64, dy):
    """(c): worst |k - y64| / (ulp_store / 2 + dy) over the tensor (<= 1 holds; NaN -> inf)."""
    kd = k.double()
    r = (kd - y64).abs() / (0.5 * ulp_store(torch.maximum(y64.abs(), kd.abs()), k.dtype) + dy)
    return float(torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).max())


def bound_abs(k, y64, dy):
    """(b): worst |k - y64| / dy."""
    r = (k.double() - y64).abs() / dy
    return float(torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).max())


# ------------------------------------------------------------------ weights --
@functools.lru_cache(maxsize=None)
def weights(dtype=torch.float64):
    """(Wx, b, Wh) gate-major (f32_split_ref.cell_weights), the weights rounded to bf16 by torch, fp32 biases."""
    Wx, b, Wh = R.cell_weights(dtype=torch.float32)
    return Wx.to(BF).to(dtype), b.to(dtype), Wh.to(BF).to(dtype)


def _convT(dz, W, cin):
    """The transposed 3x3 convolution (the dgrad): dz (B,512,w,h) -> (B,cin,w,h)."""
    return torch.nn.grad.conv2d_input((dz.shape[0], cin) + tuple(dz.shape[2:]), W, dz, padding=1)


# ---------------------------------------------------------- fp64 references --
def fwd_step(x, hp, cp):
    """One forward step in fp64 on the stored operands x (B,64,w,h), hp, cp (B,128,w,h), reference orientation.
    -> {"gates" (B,4,128,w,h), "c", "h"} and the (b)/(c) allowances {"d_gates", "d_c", "d_h"}."""
    Wx, b, Wh = weights()
    B, _, w, h = x.shape
    Z = (F.conv2d(x, Wx, b, padding=1) + F.conv2d(hp, Wh, None, padding=1)).reshape(B, 4, 128, w, h)
    S = (F.conv2d(x.abs(), Wx.abs(), b.abs(), padding=1) + F.conv2d(hp.abs(), Wh.abs(), None, padding=1))
    dZ = (KZ * U * S).reshape(B, 4, 128, w, h)
    gi, gf, go = torch.sigmoid(Z[:, 0]), torch.sigmoid(Z[:, 1]), torch.sigmoid(Z[:, 3])
    gg = torch.tanh(Z[:, 2])
    d_i, d_f, d_o, d_g = dZ[:, 0] / 4 + A_SIG, dZ[:, 1] / 4 + A_SIG, dZ[:, 3] / 4 + A_SIG, dZ[:, 2] + A_TANH
    c = gf * cp + gi * gg
    d_c = cp.abs() * d_f + gg.abs() * d_i + gi * d_g + 3 * U * ((gf * cp).abs() + (gi * gg).abs())
    tc = torch.tanh(c)
    hh = go * tc
    # h = o tanh_fast(c_kernel): the kernel's c within d_c of c64 (tanh' <= 1), tanh_fast within A_TANH, one product
    d_h = tc.abs() * d_o + go * (d_c + A_TANH) + U * hh.abs()
    return {"gates": torch.stack([gi, gf, gg, go], 1), "c": c, "h": hh,
            "d_gates": torch.stack([d_i, d_f, d_g, d_o], 1), "d_c": d_c, "d_h": d_h}


def bwd_step(g, cp, cc, dO, dz_next, dhT, dc, d_dc):
    """One BPTT step in fp64: g (B,4,128,w,h) the stored gates, cp = c_{t-1}, cc = c_t (stored, or None: recomputed
    from g and cp as the frame-resident kernels do), dO (B,128,w,h), dz_next (B,512,w,h) the kernel's own bf16
    dZ_{t+1} or None, dhT the carried cotangent (last step) or None, dc the fp64 carry and d_dc its allowance.
    -> dz (B,4,128,w,h), its allowance d_dz, the carry out (dc, d_dc)."""
    _, _, Wh = weights()
    gi, gf, gg, go = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    dh, S = dO.clone(), dO.abs()
    if dz_next is not None:
        dh, S = dh + _convT(dz_next, Wh, 128), S + _convT(dz_next.abs(), Wh.abs(), 128)
    if dhT is not None:
        dh, S = dh + dhT, S + dhT.abs()
    d_dh = KD * U * S
    if cc is None:
        cc = gf * cp + gi * gg
    tc = torch.tanh(cc)
    d_tc = A_TANH + 3 * U * cc.abs()   # tanh_fast, and the recomputed c's two products and sum (tanh' <= 1)
    term = dh * go * (1 - tc * tc)
    d_term = d_dh * go * (1 - tc * tc) + dh.abs() * go * 2 * tc.abs() * d_tc + 4 * U * term.abs()
    dcc = dc + term
    d_dcc = d_dc + d_term + U * dcc.abs()
    dout = dh * tc * (1 - go) * go
    d_out = d_dh * tc.abs() * (1 - go) * go + dh.abs() * (1 - go) * go * d_tc + 4 * U * dout.abs()
    di = dcc * gg * (1 - gi) * gi
    df = dcc * cp * (1 - gf) * gf
    dg = dcc * gi * (1 - gg * gg)
    d_i = d_dcc * (gg * (1 - gi) * gi).abs() + 4 * U * di.abs()
    d_f = d_dcc * (cp * (1 - gf) * gf).abs() + 4 * U * df.abs()
    d_g = d_dcc * (gi * (1 - gg * gg)).abs() + 4 * U * dg.abs()
    dcn = dcc * gf
    return (torch.stack([di, df, dg, dout], 1), torch.stack([d_i, d_f, d_g, d_out], 1), dcn,
            d_dcc * gf + U * dcn.abs())


def _g2r(t, B, h, w):
    return R.gates_to_ref(t.double(), B, h, w)


def _r(t, B, h, w):
    return R.to_ref(t.double(), B, h, w)


def check(o, cap, a_div=1, what="", backward=True, wgrad_only=False):
    """Every bound on one run's stored buffers ``o`` (row-major, kernel element types; see standin / the GPU
    test's _learner): -> (report {observable: {"a" | "b" | "c": err / gate, "d": share}}, failures [(bound,
    observable, text)]).  a_div: (a)'s gates divided by it (4 for the CPU stand-ins)."""
    T, B, h, w = o["T"], o["B"], o["h"], o["w"]
    rep, bad = {}, []

    def put(obs, bound, ratio, ok=None, fmt="err/gate"):
        rep.setdefault(obs, {})[bound] = ratio
        print(f"[bf16lstm] {what} {obs} ({bound}): {fmt} {ratio:.3e}")
        if not (ratio <= 1.0 if ok is None else ok):
            bad.append((bound, obs, f"{what} {obs}: bound ({bound}) {fmt} {ratio:.3e}"))

    def put_a(obs, got, ref, gate):
        put(obs, "a", V.rel(got, ref) / (gate / a_div))

    def put_d(obs, k, y64):
        ok, s = share_ok(k, y64, cap)
        put(obs, "d", s, ok, "mismatch share")

    xh = o["xh"]
    x = _r(xh[:T, :, :64], B, h, w)
    hprev = _r(xh[:T, :, 64:], B, h, w)
    hnext = R.to_ref(xh[1:, :, 64:].contiguous(), B, h, w)   # bf16
    C = _r(o["c"], B, h, w)
    gk = R.gates_to_ref(o["gates"], B, h, w)                 # stored type
    if not wgrad_only:
        f = [fwd_step(x[t], hprev[t], C[t]) for t in range(T)]
        st = lambda k: torch.stack([s[k] for s in f])   # noqa: E731
        put_a("c", C[1:], st("c"), GATE_A)
        put("c", "b", bound_abs(C[1:], st("c"), st("d_c")))
        put("gates", "c", bound_c(gk, st("gates"), st("d_gates")))
        put("h", "c", bound_c(hnext, st("h"), st("d_h")))
        if gk.dtype != torch.float32:
            put_d("gates", gk, st("gates"))
        put_d("h", hnext, st("h"))
    if not backward:
        return rep, bad
    _, _, Wh = weights()
    Wx = weights()[0]
    g64 = gk.double()
    dO = _r(o["dO"], B, h, w)
    dzk = R.to_ref(o["dz"], B, h, w)                          # (T,B,512,w,h) bf16, channel 4*ch + gate
    dzk_g = R.gates_to_ref(o["dz"], B, h, w)                  # (T,B,4,128,w,h) bf16
    dz_gm = dzk_g.double().reshape(T, B, 512, w, h)           # gate-major rows g*128 + ch, as the weights'
    dxk = R.to_ref(o["dx"], B, h, w)
    del dzk
    dhT = None if o.get("dhT") is None else _r(o["dhT"], B, h, w)
    dc = torch.zeros(B, 128, w, h, dtype=torch.float64) if o.get("dcT") is None else _r(o["dcT"], B, h, w)
    d_dc = torch.zeros_like(dc)
    dz64, d_dz, dx64, d_dx = [None] * T, [None] * T, [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        cc = C[t + 1] if o["ccur"] == "stored" else None
        dz64[t], d_dz[t], dc, d_dc = bwd_step(g64[t], C[t], cc, dO[t], dz_gm[t + 1] if t + 1 < T else None,
                                              dhT if t == T - 1 else None, dc, d_dc)
        dx64[t] = _convT(dz_gm[t], Wx, 64)
        d_dx[t] = KD * U * _convT(dz_gm[t].abs(), Wx.abs(), 64)
    dz64, d_dz, dx64, d_dx = (torch.stack(v) for v in (dz64, d_dz, dx64, d_dx))
    if not wgrad_only:
        put("dz", "c", bound_c(dzk_g, dz64, d_dz))
        put_d("dz", dzk_g, dz64)
        put("dx", "c", bound_c(dxk, dx64, d_dx))
        put_d("dx", dxk, dx64)
        put_a("dh0", _r(o["dh0"], B, h, w), _convT(dz_gm[0], Wh, 128), GATE_A)
        put_a("dc0", _r(o["dc0"], B, h, w), dc, GATE_A)
        gb_sum = dz64.reshape(T, B, 512, w, h).sum((0, 1, 3, 4))       # the unrounded fp64 dZ
        gb_rnd = dz_gm.sum((0, 1, 3, 4))                               # the stored bf16 dZ
        e_sum, e_rnd = V.rel(o["grads"]["gb"], gb_sum) / GATE_BSUM, V.rel(o["grads"]["gb"], gb_rnd) / GATE_A
        put("gb", "a", (e_sum if o["gb_sum"] == "fp32" else min(e_sum, e_rnd)) * a_div)
        put("gb2", "a", V.rel(o["gb2"], dx64.sum((0, 1, 3, 4))) / GATE_BSUM * a_div)
    fl = lambda t: t.reshape(T * B, *t.shape[2:])   # noqa: E731
    put_a("gWx", o["grads"]["gWx"], conv2d_weight(fl(x), Wx.shape, fl(dz_gm), padding=1), GATE_A)
    put_a("gWh", o["grads"]["gWh"], conv2d_weight(fl(hprev), Wh.shape, fl(dz_gm), padding=1), GATE_A)
    return rep, bad


# ------------------------------------------------------ CPU case inputs ------
@functools.lru_cache(maxsize=None)
def case_inputs(T, B, H, W, state):
    """Inputs built like the GPU test's, all row-major kernel layouts: x (T, M, 64) bf16 the (oracle's) vision
    features of detinit frames, h0 / c0 (M, 128) fp32 or None, dO (T, M, 128) fp32 the oracle head's cotangent of
    a plain fp32 recurrence's h_t, dhT / dcT at dO's scale (state cases)."""
    params = detinit.deterministic_params(0, 18)
    P = ref_cpu.tensor_params(params, requires_grad=False)
    h, w = ref_cpu.grid_of(H, W)
    M = B * h * w
    X = R.frames(T, B, H, W, FRAME_SCALE)
    with torch.no_grad():
        xr = torch.stack([ref_cpu.vision_cnn(P, X[t], "bf16") for t in range(T)]).to(BF)     # (T,B,64,w,h)
    h0 = c0 = dhT = dcT = None
    if state:
        h0, c0 = (t.reshape(M, 128) for t in R.state_in(B, h, w))
    W32 = weights(torch.float32)
    f32 = R.recur_fwd(W32, xr.float(), None if h0 is None else R.to_ref(h0.to(BF).float(), B, h, w),
                      None if c0 is None else R.to_ref(c0, B, h, w))
    S = ref_cpu.spatial_basis(h, w)
    Gl, Gv = (torch.from_numpy(detinit.cotangent(s, (T, B, 18))) for s in (2, 3))
    dO = []
    for t in range(T):
        O = f32["h"][t].clone().requires_grad_(True)
        lg, vl, _ = ref_cpu._head(P, O.transpose(1, 3), S, 4, None, None)
        (gO,) = torch.autograd.grad((lg * Gl[t]).sum() + (vl * Gv[t]).sum(), O)
        dO.append(gO)
    dO = R.from_ref(torch.stack(dO)).contiguous()
    if state:
        dhT, dcT = (t.reshape(M, 128) for t in R.state_cot(B, h, w, float(dO.abs().max())))
    return {"T": T, "B": B, "h": h, "w": w, "x": R.from_ref(xr).contiguous(), "h0": h0, "c0": c0, "dO": dO,
            "dhT": dhT, "dcT": dcT}


# --------------------------------------------------------- CPU stand-in ------
def sigm_model(x, off=0.0):
    """float32 model of sigm_fast: 1 / (1 + exp2(-x * log2e))."""
    return 1.0 / (1.0 + torch.exp2(x * torch.tensor(-LOG2E, dtype=torch.float32))) + off


def tanh_model(x):
    return 2.0 * sigm_model(2.0 * x) - 1.0


def _gemm_tiles(Wm, cols, acc=None, tile=32):
    """acc + Wm (R, K) @ cols (N, K, L), K in ``tile``-wide pieces summed one by one in fp32."""
    for k0 in range(0, Wm.shape[1], tile):
        p = torch.matmul(Wm[:, k0:k0 + tile], cols[:, k0:k0 + tile])
        acc = p if acc is None else acc + p
    return acc


def _conv_f32(inp, Wt, order, acc=None):
    """3x3 same convolution in fp32 of inp (N,C,w,h) with Wt (R,C,3,3): torch's order ("whole"), or K = C*9 in
    32-wide tiles summed in fp32 ("tiles").  -> (N,R,w,h) (+ acc)."""
    if order == "whole":
        y = F.conv2d(inp, Wt, None, padding=1)
        return y if acc is None else acc + y
    N, _, w, h = inp.shape
    cols = F.unfold(inp, 3, padding=1)
    a = None if acc is None else acc.reshape(N, Wt.shape[0], w * h)
    return _gemm_tiles(Wt.reshape(Wt.shape[0], -1), cols, a).reshape(N, Wt.shape[0], w, h)


def _flipT(Wt):
    """The dgrad's weights: conv2d_input(W, dz) = conv2d(dz, _flipT(W))."""
    return Wt.transpose(0, 1).flip(2, 3).contiguous()


def standin(case, order="whole", defect=None, ccur="recomputed"):
    """A kernel stand-in in float32 torch on case_inputs(*case): the stored buffers a run leaves, row-major,
    in the kernels' element types (the dict check() reads).  defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    ci = case_inputs(*case)
    T, B, h, w = ci["T"], ci["B"], ci["h"], ci["w"]
    M = B * h * w
    Wx, b, Wh = weights(torch.float32)
    ref = lambda t: R.to_ref(t, B, h, w)   # noqa: E731
    x = ref(ci["x"].float())                                                     # (T,B,64,w,h)
    hs = [torch.zeros(B, 128, w, h, dtype=BF) if ci["h0"] is None else ref(ci["h0"].to(BF))]
    cs = [torch.zeros(B, 128, w, h) if ci["c0"] is None else ref(ci["c0"])]
    G16, G32 = [], []
    sig_off = 1e-5 if defect == "sigma_1e-5" else 0.0
    for t in range(T):
        hp = hs[t].float()
        if defect == "stale_row" and t >= 1:   # the halo row a neighbour band published one step late
            row = 5 if h >= 21 else h // 2
            hp = hp.clone()
            hp[..., row] = hs[t - 1].float()[..., row]
        Z = _conv_f32(hp, Wh, order, _conv_f32(x[t], Wx, order))
        if defect == "border_taps":   # the taps of the image's last column: kernel column offset +1 (reference dim 2)
            hm, Wm = torch.zeros_like(hp), torch.zeros_like(Wh)
            hm[:, :, w - 1], Wm[:, :, 2] = hp[:, :, w - 1], Wh[:, :, 2]
            Z = Z - F.conv2d(hm, Wm, None, padding=1)
        Z = (Z + b[None, :, None, None]).reshape(B, 4, 128, w, h)
        gi, gf, go = (sigm_model(Z[:, k], sig_off) for k in (0, 1, 3))
        gg = tanh_model(Z[:, 2])
        c = gf * cs[t] + gi * gg
        hh = go * tanh_model(c)
        g32 = torch.stack([gi, gf, gg, go], 1)
        G32.append(g32), G16.append(g32.to(F16)), cs.append(c)
        hs.append(V.trunc_bf16(hh) if defect == "trunc_h" else hh.to(BF))
    o = {"T": T, "B": B, "h": h, "w": w, "ccur": ccur, "gb_sum": "fp32"}
    hrows = torch.stack([R.from_ref(t) for t in hs])                              # (T+1, M, 128) bf16
    xrows = torch.cat([ci["x"], torch.zeros(1, M, 64, dtype=BF)])
    o["xh"] = torch.cat([xrows, hrows], dim=2)
    o["c"] = torch.stack([R.from_ref(t) for t in cs]).contiguous()
    o["gates"] = torch.stack([R.gates_from_ref(t) for t in G16]).contiguous()
    o["hT"], o["cT"] = hrows[-1].float(), o["c"][-1]
    # ---- BPTT
    dO = ref(ci["dO"])
    dc = torch.zeros(B, 128, w, h) if ci["dcT"] is None else ref(ci["dcT"])
    WhT, WxT = _flipT(Wh), _flipT(Wx)
    DZ, DX = [None] * T, [None] * T
    gb, gb2 = torch.zeros(512), torch.zeros(64)
    for t in range(T - 1, -1, -1):
        dh = dO[t] if t == T - 1 else _conv_f32(DZ[t + 1].float(), WhT, order, dO[t])
        if t == T - 1 and ci["dhT"] is not None:
            dh = dh + ref(ci["dhT"])
        g = (G32 if defect == "gates_fp32_bwd" else G16)[t].float()
        gi, gf, gg, go = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
        cc = gf * cs[t] + gi * gg if ccur == "recomputed" else cs[t + 1]
        tc = tanh_model(cc)
        dcc = dc + dh * go * (1 - tc * tc)
        dz = torch.stack([dcc * gg * (1 - gi) * gi, dcc * cs[t] * (1 - gf) * gf, dcc * gi * (1 - gg * gg),
                          dh * tc * (1 - go) * go], 1).reshape(B, 512, w, h)
        dc = dcc * gf
        gb = gb + dz.sum((0, 2, 3))
        DZ[t] = V.trunc_bf16(dz) if defect == "trunc_dz" else dz.to(BF)
        dx = _conv_f32(DZ[t].float(), WxT, order)
        gb2 = gb2 + dx.sum((0, 2, 3))
        DX[t] = dx.to(BF)
    o["dO"], o["dhT"], o["dcT"] = ci["dO"], ci["dhT"], ci["dcT"]
    to_rows = lambda t: R.gates_from_ref(t.reshape(B, 4, 128, w, h))   # noqa: E731
    o["dz"] = torch.stack([to_rows(t) for t in DZ]).contiguous()
    o["dx"] = torch.stack([R.from_ref(t) for t in DX]).contiguous()
    o["dh0"] = R.from_ref(_conv_f32(DZ[0].float(), WhT, order)).contiguous()
    o["dc0"] = R.from_ref(dc).contiguous()
    # ---- weight gradient: K = the T*B*P pixel rows
    dz_all = torch.stack(DZ).float().reshape(T * B, 512, w, h)
    xh_all = torch.cat([x, torch.stack(hs[:T]).float()], dim=2).reshape(T * B, 192, w, h)
    if order == "whole" and defect != "splitk_bf16":
        gWx = conv2d_weight(xh_all[:, :64], Wx.shape, dz_all, padding=1)
        gWh = conv2d_weight(xh_all[:, 64:], Wh.shape, dz_all, padding=1)
    else:
        cols = F.unfold(xh_all, 3, padding=1).permute(0, 2, 1).reshape(-1, 192 * 9)     # (rows, 1728)
        dzr = dz_all.permute(0, 2, 3, 1).reshape(-1, 512)                               # (rows, 512), same row order
        rows = cols.shape[0]
        nsplit = 8 if defect == "splitk_bf16" else 1
        per = (rows + nsplit - 1) // nsplit
        acc = None
        for s0 in range(0, rows, per):
            part = None
            for k0 in range(s0, min(s0 + per, rows), 32):
                k1 = min(k0 + 32, s0 + per, rows)
                p = dzr[k0:k1].t() @ cols[k0:k1]
                part = p if part is None else part + p
            if defect == "splitk_bf16":
                part = part.to(BF).float()
            acc = part if acc is None else acc + part
        gW = acc.reshape(512, 192, 3, 3)
        gWx, gWh = gW[:, :64].contiguous(), gW[:, 64:].contiguous()
    o["grads"] = {"gWx": gWx, "gWh": gWh, "gb": gb}
    o["gb2"] = gb2
    return o


# ------------------------------------------------------ the cell entry ------
@functools.lru_cache(maxsize=None)
def cell_inputs(B, h, w):
    """f32_split_ref.cell_case's inputs (same seeds and scales), NHWC as the entry takes them."""
    return {"x": R.rnd((B, h, w, 64), 1, 3.0), "h0": R.rnd((B, h, w, 128), 2), "c0": R.rnd((B, h, w, 128), 3),
            "dh1": R.rnd((B, h, w, 128), 4), "dc1": R.rnd((B, h, w, 128), 5)}


def _gate_bwd(dh, dc, g, cp, cc, tanh, assoc=0):
    """The gate backward in the operands' dtype -> (dz (B,4,128,w,h), dc out).  assoc: one of three association
    orders of the same products (the same value in exact arithmetic, other roundings in fp32)."""
    gi, gf, gg, go = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    tc = tanh(cc)
    if assoc == 0:
        dcc = dc + dh * go * (1 - tc * tc)
        dz = [dcc * gg * (1 - gi) * gi, dcc * cp * (1 - gf) * gf, dcc * gi * (1 - gg * gg), dh * tc * (1 - go) * go]
    elif assoc == 1:
        dcc = dc + dh * (go * (1 - tc * tc))
        dz = [dcc * (gg * ((1 - gi) * gi)), dcc * (cp * ((1 - gf) * gf)), dcc * (gi * (1 - gg * gg)),
              dh * (tc * ((1 - go) * go))]
    else:
        dcc = dc + (dh * (1 - tc * tc)) * go
        dz = [(dcc * gi) * ((1 - gi) * gg), (dcc * gf) * ((1 - gf) * cp), (dcc * (1 - gg * gg)) * gi,
              (dh * go) * ((1 - go) * tc)]
    return torch.stack(dz, 1), dcc * gf


def cell_ref(io, B, h, w, c1_kernel, gate_dtype):
    """The cell entry's references and gates.  The entry's inputs are known (x, h0 rounded to bf16 by torch as
    cell_xh does; c0, dh1, dc1 fp32), its h1 / c1 come back in fp32: (a) on both.  Its gate activations
    (``gate_dtype``) and its dZ (bf16) never leave its workspace, so the reference rounds its OWN fp64 gates and
    dZ (one rounding each) and reads the kernel's c1 (``c1_kernel``, (M, 128): the ``ccur`` its gate backward
    loads); what then differs from a correct kernel is the handful of elements whose fp32 value rounds the other
    way.  e_flip[obs] is the change of the fp64 result when those roundings are taken from a float32 evaluation
    instead, computed from the reference alone: the LARGEST over six evaluations (torch's activations and the
    fast-activation model, each with three association orders of the gate backward's products) -- one
    evaluation is not a yardstick, a single large dZ element on a rounding boundary decides its figure
    (vision_bf16_ref.fused_gw1_ref).  The gate is 4 e_flip + GATE_A, as vision_bf16_ref (e).
    -> (ref {h1, c1, dx, dh0, dc0, gWx, gWh, gb} in the kernels' layouts, gate {obs: float})."""
    M = B * h * w
    Wx, b, Wh = weights()
    r = lambda t: R.to_ref(t.reshape(M, -1), B, h, w)   # noqa: E731
    xb, hb = r(io["x"]).to(BF).double(), r(io["h0"]).to(BF).double()
    c0, dh1, dc1 = (r(io[k]).double() for k in ("c0", "dh1", "dc1"))
    cc = R.to_ref(c1_kernel, B, h, w).double()
    f = fwd_step(xb, hb, c0)

    def outs(g, dz, dc0):
        dzb = dz.reshape(B, 512, w, h)
        return {"dx": _convT(dzb, Wx, 64), "dh0": _convT(dzb, Wh, 128), "dc0": dc0,
                "gWx": conv2d_weight(xb, Wx.shape, dzb, padding=1), "gWh": conv2d_weight(hb, Wh.shape, dzb, padding=1),
                "gb": dzb.sum((0, 2, 3))}

    g = rne(f["gates"], gate_dtype).double()
    dz, dc0 = _gate_bwd(dh1, dc1, g, c0, cc, torch.tanh)
    ex = outs(g, rne(dz, BF).double(), dc0)
    Wx32, b32, Wh32 = weights(torch.float32)
    Z = F.conv2d(xb.float(), Wx32, b32, padding=1) + F.conv2d(hb.float(), Wh32, None, padding=1)
    Z = Z.reshape(B, 4, 128, w, h)
    e_flip = {k: 0.0 for k in ex}
    for sig, tanh in ((torch.sigmoid, torch.tanh), (sigm_model, tanh_model)):
        g32 = torch.stack([sig(Z[:, 0]), sig(Z[:, 1]), tanh(Z[:, 2]), sig(Z[:, 3])], 1).to(gate_dtype).float()
        for assoc in range(3):
            dz32, dc32 = _gate_bwd(dh1.float(), dc1.float(), g32, c0.float(), cc.float(), tanh, assoc)
            alt = outs(g32.double(), dz32.to(BF).double(), dc32.double())
            for k in ex:
                e_flip[k] = max(e_flip[k], V.rel(alt[k], ex[k]))
    ref = {"h1": R.from_ref(f["h"]), "c1": R.from_ref(f["c"]), "dx": R.from_ref(ex["dx"]), "dh0": R.from_ref(ex["dh0"]),
           "dc0": R.from_ref(ex["dc0"]), "gWx": ex["gWx"], "gWh": ex["gWh"], "gb": ex["gb"]}
    gate = {"h1": GATE_A, "c1": GATE_A}
    gate.update({k: 4 * e_flip[k] + GATE_A for k in ex})
    return ref, gate


def cqm4_direct(rows, P):
    """A (B*P, 128) row-major tensor written into channel-quad-major slices, element by element, by the header's
    map (the round-trip test's direct implementation)."""
    out = torch.empty_like(rows).reshape(-1, P * 128)
    for b in range(rows.shape[0] // P):
        for pp in range(P):
            for ch in range(128):
                out[b, ((ch >> 2) * P + pp) * 4 + (ch & 3)] = rows[b * P + pp, ch]
    return out.reshape(rows.shape)


def cqmg_direct(rows, P):
    out = torch.empty_like(rows).reshape(-1, P * 512)
    for b in range(rows.shape[0] // P):
        for pp in range(P):
            for ch in range(128):
                for gate in range(4):
                    out[b, ((ch >> 2) * P + pp) * 16 + (ch & 3) * 4 + gate] = rows[b * P + pp, 4 * ch + gate]
    return out.reshape(rows.shape)


assert math.isclose(U, 5.960464477539063e-08)
assert np.float32(LOG2E) == np.float32(1.4426950408889634)
