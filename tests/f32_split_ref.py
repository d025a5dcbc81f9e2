"""fp64 references, the two-part emulation and the CPU stand-in cases shared by
the fp32 split-product tests (test_f32_split_emulation.py on the CPU,
test_gpu_f32_split.py on the GPU).

Every large GEMM of the fp32 path multiplies fp32 operands on the bf16 MFMA by
cutting each into hi + mid + lo bf16 parts and summing six part products in fp32
(AAA_F32_SPLIT6, csrc/gemm.h SPLIT6, csrc/recur_f32.h k_split_frag): "fp32
accuracy".  A kernel that lost a lo part in one operand moves the recurrence's
h by about 1e-5 and a backward GEMM's result by about 2e-6 -- inside the 1e-4
gate of every end-to-end test, and below the fp32 oracle's own gradient error.
``e2[site, observable]`` is the error such a kernel would make on a case's own
inputs: the same formulas in fp64 with ONE operand site of ONE GEMM replaced by
its first two bf16 parts (``split2``).  The GPU tests hold a kernel to e2 / 2
against fp64 evaluated on the kernel's own saved inputs, for every site that
reaches the observable; the CPU test holds plain torch float32 to e2 / 4.

Layouts.  The kernels keep images pixel-major, channel fastest: (B*h*w, C) rows
of an NHWC (B, h, w, C) tensor.  The references run torch's NCHW convolutions in
the reference implementation's orientation (B, C, w, h) (attention.py:179's
transpose; tests/test_gpu_components.py test_convlstm_cell_abi_state_grads):
``to_ref`` / ``from_ref`` are the permutation (0, 3, 2, 1) either way.

Quantities and sites (Z = the 512 gate pre-activations, gate-major here, row
4*ch + gate in the kernels' exports):
  recurrence   Z_t = Wx * x_t + b + Wh * h_{t-1}; i, f, o = sigmoid, c~ = tanh;
               c_t = f c_{t-1} + i c~;  h_t = o tanh(c_t)          sites: W, xh
  BPTT         dh_t = dO_t + Wh^T * dZ_{t+1} (dh_{T-1} = dO + dhT)
               dZ_t from (dh_t, dc_t, gates_t, c_t, c_{t-1}): _GateCellF16.backward's formulas
               dx_t = Wx^T * dZ_t                                  sites: dgrad.W, dgrad.dZ
               gWx = sum_t dZ_t (x) x_t, gWh = sum_t dZ_t (x) h_{t-1}
                                                                   sites: wgrad.XH, wgrad.dZ
  vision CNN   y1 = conv1(x), y2 = conv2(y1)                       sites: conv1.W, conv1.x, conv2.W, conv2.y1
               dy1 = conv2^T(dy2)                                  sites: dgrad2.W, dgrad2.dy2
               gW2 = dy2 (x) y1, gW1 = dy1 (x) x                   sites: wgrad2.y1, wgrad2.dy2, wgrad1.x, wgrad1.dy1
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from helpers import detinit, rel_err
from oracle import ref_cpu

GATES = "ifco"
LSTM = "vision.vision_lstm."
CNN = "vision.vision_cnn."

FWD_SITES = ("W", "xh")
DGRAD_SITES = ("dgrad.W", "dgrad.dZ")
WGRAD_SITES = ("wgrad.XH", "wgrad.dZ")
# observable -> the sites that reach it
FWD_REACH = {"h": FWD_SITES, "c": FWD_SITES}
BWD_REACH = {"dx": DGRAD_SITES, "dh0": DGRAD_SITES, "gWx": WGRAD_SITES, "gWh": WGRAD_SITES}
CNN_REACH = {"y1": ("conv1.W", "conv1.x"), "y2": ("conv2.W", "conv2.y1"), "dy1": ("dgrad2.W", "dgrad2.dy2"),
             "gW2": ("wgrad2.y1", "wgrad2.dy2"), "gW1": ("wgrad1.x", "wgrad1.dy1")}

# (T, B, H, W, carried state): the smallest shapes at which the frame-group kernels can go wrong
# (tests/test_gpu_f32_frames.py): P = 121 (padding columns), a ragged second group of eight frames,
# P = 64 (kPsZP, the staging aliases the x image), and a non-zero h0 / c0 (the t = 0 h-part is not skipped)
UNROLL_CASES = [(3, 2, 84, 84, False), (2, 9, 84, 84, False), (4, 3, 64, 64, False), (3, 2, 84, 84, True)]
# the weight gradient's K-loop edges of tests/test_gpu_wgrad_paired.py CASES at 75, 363 and 540 rows (the single
# step of the 540-row case starts from a carried state: from zeros its h operand, and so gWh, is identically zero)
WGRAD_EDGE_CASES = [(3, 1, 36, 36, False), (3, 1, 84, 84, False), (1, 1, 210, 160, True)]
CELL_CASES = [(2, 11, 11), (3, 7, 13), (1, 21, 21)]
CNN_CASES = [(2, 84, 84), (2, 80, 100)]   # 80x100: an odd conv1 map (19 rows)
FRAME_SCALE = 0.37   # integer-valued frames are exact in bf16: cutting conv1's x would change nothing


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def split2(x: torch.Tensor) -> torch.Tensor:
    """fp32 x cut to its first two bf16 parts, as fp64."""
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16).float()
    mid = (x - hi).to(torch.bfloat16).float()
    return hi.double() + mid.double()


def _cut(x: torch.Tensor) -> torch.Tensor:
    """The operand a kernel without lo parts would multiply: x as the fp32 value the kernel holds, two parts of it."""
    return split2(x.float())


def to_ref(x, B, h, w):
    """(..., B*h*w, C) pixel-major rows -> (..., B, C, w, h)."""
    lead, C = tuple(x.shape[:-2]), x.shape[-1]
    n = len(lead)
    return x.reshape(*lead, B, h, w, C).permute(*range(n), n, n + 3, n + 2, n + 1).contiguous()


def from_ref(x):
    """(..., B, C, w, h) -> (..., B*h*w, C)."""
    n = x.dim() - 4
    B, C, w, h = x.shape[n:]
    return x.permute(*range(n), n, n + 3, n + 2, n + 1).reshape(*x.shape[:n], B * h * w, C)


def gates_to_ref(g, B, h, w):
    """The kernels' (..., B*h*w, 512) gate rows (4*ch + gate) -> (..., B, 4, 128, w, h)."""
    r = to_ref(g, B, h, w)                                  # (..., B, 512, w, h), channel 4*ch + gate
    n = r.dim() - 4
    return r.reshape(*r.shape[:n], B, 128, 4, w, h).transpose(n + 1, n + 2).contiguous()


def gates_from_ref(g):
    """(..., B, 4, 128, w, h) -> (..., B*h*w, 512), row 4*ch + gate."""
    n = g.dim() - 5
    B, _, _, w, h = g.shape[n:]
    return from_ref(g.transpose(n + 1, n + 2).reshape(*g.shape[:n], B, 512, w, h))


def cell_weights(params=None, dtype=torch.float64):
    """(Wx (512,64,3,3), b (512), Wh (512,128,3,3)), gate-major rows g*128 + ch, from a name -> array dict."""
    P = params if params is not None else detinit.deterministic_params(0, 18)
    t = lambda k: torch.as_tensor(np.ascontiguousarray(P[k])).float()   # noqa: E731
    Wx = torch.cat([t(f"{LSTM}Wx{g}.weight") for g in GATES])
    b = torch.cat([t(f"{LSTM}Wx{g}.bias") for g in GATES])
    Wh = torch.cat([t(f"{LSTM}Wh{g}.weight") for g in GATES])
    return Wx.to(dtype), b.to(dtype), Wh.to(dtype)


def cnn_weights(params=None, dtype=torch.float64):
    P = params if params is not None else detinit.deterministic_params(0, 18)
    return tuple(torch.as_tensor(np.ascontiguousarray(P[CNN + k])).float().to(dtype)
                 for k in ("0.weight", "0.bias", "1.weight", "1.bias"))


def flat_cell_grads(r):
    """A bptt() result's 12 ConvLSTM gradients in state_dict order (Wx{g}.weight, Wx{g}.bias, Wh{g}.weight for
    g in i, f, c, o), flat -- aaa_convlstm_cell_bwd's ``grads``."""
    out = []
    for k in range(4):
        s = slice(128 * k, 128 * (k + 1))
        out += [r["gWx"][s].reshape(-1), r["gb"][s].reshape(-1), r["gWh"][s].reshape(-1)]
    return torch.cat(out)


def split_cell_grads(flat):
    """The inverse for a flat (possibly device) gradient: {"gWx", "gb", "gWh"} gate-major, on the host."""
    flat = flat.detach().cpu()
    nx, nh = 128 * 64 * 9, 128 * 128 * 9
    gx, gb, gh, off = [], [], [], 0
    for _ in range(4):
        gx.append(flat[off:off + nx].reshape(128, 64, 3, 3)); off += nx
        gb.append(flat[off:off + 128]); off += 128
        gh.append(flat[off:off + nh].reshape(128, 128, 3, 3)); off += nh
    return {"gWx": torch.cat(gx), "gb": torch.cat(gb), "gWh": torch.cat(gh)}


# ------------------------------------------------------------ recurrence ----
def recur_fwd(W, x, h0=None, c0=None, site=None):
    """The recurrence, free-running from x (T,B,64,w,h) and (h0, c0) (B,128,w,h) or zeros, in W's dtype.
    site "W" / "xh": that operand of the gate GEMM cut to two bf16 parts (fp64 only).
    -> {"gates" (T,B,4,128,w,h) post-activation, "c" (T,B,128,w,h), "h" (T,B,128,w,h)}."""
    Wx, b, Wh = W
    dt = Wx.dtype
    assert site in (None,) + FWD_SITES and (site is None or dt == torch.float64)
    T, B, _, w, h = x.shape
    hp = torch.zeros(B, 128, w, h, dtype=dt) if h0 is None else h0.to(dt)
    cp = torch.zeros(B, 128, w, h, dtype=dt) if c0 is None else c0.to(dt)
    if site == "W":
        Wx, Wh = _cut(Wx), _cut(Wh)
    G, Cs, Hs = [], [], []
    for t in range(T):
        xt, ht = x[t].to(dt), hp
        if site == "xh":
            xt, ht = _cut(xt), _cut(ht)
        z = (F.conv2d(xt, Wx, b, padding=1) + F.conv2d(ht, Wh, None, padding=1)).reshape(B, 4, 128, w, h)
        gi, gf, go = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.sigmoid(z[:, 3])
        gc = torch.tanh(z[:, 2])
        cp = gf * cp + gi * gc
        hp = go * torch.tanh(cp)
        G.append(torch.stack([gi, gf, gc, go], dim=1)), Cs.append(cp), Hs.append(hp)
    return {"gates": torch.stack(G), "c": torch.stack(Cs), "h": torch.stack(Hs)}


def bptt(W, x, hprev, gates, cprev, c, dO, dhT=None, dcT=None, site=None):
    """BPTT from saved products, in W's dtype: x (T,B,64,w,h); hprev / cprev (T,B,128,w,h) = h_{t-1} / c_{t-1}
    (slot 0 the incoming state); gates (T,B,4,128,w,h); c = c_t; dO = the readout's cotangent of h_t; dhT / dcT
    the carried cotangents of (h_{T-1}, c_{T-1}) or None.  site: one operand of the dgrad or of the wgrad GEMM
    cut to two bf16 parts (fp64 only).
    -> {"gWx" (512,64,3,3), "gWh" (512,128,3,3), "gb" (512), "dx" (T,B,64,w,h), "dh0", "dc0" (B,128,w,h)}."""
    Wx, _, Wh = W
    dt = Wx.dtype
    assert site in (None,) + DGRAD_SITES + WGRAD_SITES and (site is None or dt == torch.float64)
    T, B, _, w, h = x.shape
    x, hprev, gates, cprev, c, dO = (t.to(dt) for t in (x, hprev, gates, cprev, c, dO))
    Wxd, Whd = (_cut(Wx), _cut(Wh)) if site == "dgrad.W" else (Wx, Wh)
    dh = torch.zeros(B, 128, w, h, dtype=dt) if dhT is None else dhT.to(dt)
    dc = torch.zeros(B, 128, w, h, dtype=dt) if dcT is None else dcT.to(dt)
    gWx, gWh, gb = torch.zeros_like(Wx), torch.zeros_like(Wh), torch.zeros(512, dtype=dt)
    dx = [None] * T
    for t in range(T - 1, -1, -1):
        dh = dh + dO[t]
        gi, gf, gc, go = gates[t, :, 0], gates[t, :, 1], gates[t, :, 2], gates[t, :, 3]
        tc = torch.tanh(c[t])
        dcc = dc + dh * go * (1 - tc * tc)
        dz = torch.stack([dcc * gc * (1 - gi) * gi, dcc * cprev[t] * (1 - gf) * gf, dcc * gi * (1 - gc * gc),
                          dh * tc * (1 - go) * go], dim=1).reshape(B, 512, w, h)
        dc = dcc * gf
        dzd = _cut(dz) if site == "dgrad.dZ" else dz
        dx[t] = conv2d_input((B, 64, w, h), Wxd, dzd, padding=1)
        dh = conv2d_input((B, 128, w, h), Whd, dzd, padding=1)
        dzw = _cut(dz) if site == "wgrad.dZ" else dz
        xw, hw = (_cut(x[t]), _cut(hprev[t])) if site == "wgrad.XH" else (x[t], hprev[t])
        gWx = gWx + conv2d_weight(xw, Wx.shape, dzw, padding=1)
        gWh = gWh + conv2d_weight(hw, Wh.shape, dzw, padding=1)
        gb = gb + dz.sum((0, 2, 3))
    return {"gWx": gWx, "gWh": gWh, "gb": gb, "dx": torch.stack(dx), "dh0": dh, "dc0": dc}


def fwd_e2(W64, x, h0, c0):
    """(exact fp64 recurrence, {(site, observable): e2})."""
    ex = recur_fwd(W64, x, h0, c0)
    e2 = {}
    for s in FWD_SITES:
        cut = recur_fwd(W64, x, h0, c0, site=s)
        for o in FWD_REACH:
            e2[s, o] = rel_err(cut[o], ex[o])
    return ex, e2


def bwd_e2(W64, *args, sites=DGRAD_SITES + WGRAD_SITES):
    """(exact fp64 BPTT of bptt(W64, *args), {(site, observable): e2}) over ``sites``."""
    ex = bptt(W64, *args)
    e2 = {}
    for s in sites:
        cut = bptt(W64, *args, site=s)
        for o, reach in BWD_REACH.items():
            if s in reach:
                e2[s, o] = rel_err(cut[o], ex[o])
    return ex, e2


# ------------------------------------------------------------ vision CNN ----
def cnn_pieces(W, x, dy2, y1_in=None, dy1_in=None, site=None):
    """conv1 (8x8, stride 4, pad 1) and conv2 (4x4, stride 2, pad 2) of x (N,3,W,H) in W's dtype, conv2's dgrad of
    dy2 and both weight gradients.  y1_in / dy1_in: the y1 conv2 and its weight gradient read, and the dy1 conv1's
    weight gradient reads (a kernel's own; default: this function's).  site: CNN_REACH's."""
    w1, b1, w2, b2 = W
    dt = w1.dtype
    assert site is None or (dt == torch.float64 and any(site in v for v in CNN_REACH.values()))
    cut = lambda name, t: _cut(t) if site == name else t   # noqa: E731
    x, dy2 = x.to(dt), dy2.to(dt)
    y1 = F.conv2d(cut("conv1.x", x), cut("conv1.W", w1), b1, stride=4, padding=1)
    y1r = y1 if y1_in is None else y1_in.to(dt)
    y2 = F.conv2d(cut("conv2.y1", y1r), cut("conv2.W", w2), b2, stride=2, padding=2)
    dy1 = conv2d_input(y1r.shape, cut("dgrad2.W", w2), cut("dgrad2.dy2", dy2), stride=2, padding=2)
    dy1r = dy1 if dy1_in is None else dy1_in.to(dt)
    gW2 = conv2d_weight(cut("wgrad2.y1", y1r), w2.shape, cut("wgrad2.dy2", dy2), stride=2, padding=2)
    gW1 = conv2d_weight(cut("wgrad1.x", x), w1.shape, cut("wgrad1.dy1", dy1r), stride=4, padding=1)
    return {"y1": y1, "y2": y2, "dy1": dy1, "gW2": gW2, "gW1": gW1, "gb2": dy2.sum((0, 2, 3)), "gb1": dy1r.sum((0, 2, 3))}


def cnn_e2(W64, x, dy2, y1_in=None, dy1_in=None):
    ex = cnn_pieces(W64, x, dy2, y1_in, dy1_in)
    e2 = {}
    for o, reach in CNN_REACH.items():
        for s in reach:
            e2[s, o] = rel_err(cnn_pieces(W64, x, dy2, y1_in, dy1_in, site=s)[o], ex[o])
    return ex, e2


# ---------------------------------------------- CPU stand-ins of the cases ----
def frames(T, B, H, W, scale=1.0):
    return torch.from_numpy(detinit.frames_u8(1234, (T, B, H, W, 3)).astype(np.float32)) * scale


def state_in(B, h, w):
    """The carried (h0, c0) of the state cases, NHWC (B,h,w,128): |h| < 1 as an o * tanh(c) is."""
    return rnd((B, h, w, 128), 31, 0.8), rnd((B, h, w, 128), 32, 1.5)


def state_cot(B, h, w, scale):
    """(dhT, dcT), NHWC: the cotangents a following call's backward would hand over, at ``scale``."""
    return rnd((B, h, w, 128), 33, scale), rnd((B, h, w, 128), 34, scale)


def _bwd_inputs(W32, x, h0, c0, dO, dhT, dcT):
    """What a kernel's backward reads, made by the fp32 forward: (x, hprev, gates, cprev, c, dO, dhT, dcT)."""
    f = recur_fwd(W32, x, h0, c0)
    z = torch.zeros_like(f["h"][0])
    hprev = torch.cat([(z if h0 is None else h0)[None], f["h"][:-1]])
    cprev = torch.cat([(z if c0 is None else c0)[None], f["c"][:-1]])
    return x, hprev, f["gates"], cprev, f["c"], dO, dhT, dcT


@functools.lru_cache(maxsize=None)
def unroll_case(T, B, H, W, state, sites=DGRAD_SITES + WGRAD_SITES):
    """One learner case on the CPU: x_t and the readout's cotangent dO_t from the fp32 oracle on detinit weights
    and frames, then the exact / cut / fp32 recurrence and BPTT on those inputs; read-only, shared."""
    params = detinit.deterministic_params(0, 18)
    P = ref_cpu.tensor_params(params, requires_grad=False)
    h, w = ref_cpu.grid_of(H, W)
    X = frames(T, B, H, W)
    with torch.no_grad():
        x = torch.stack([ref_cpu.vision_cnn(P, X[t]) for t in range(T)])          # (T,B,64,w,h)
    h0 = c0 = None
    if state:
        h0, c0 = (to_ref(t.reshape(B * h * w, 128), B, h, w) for t in state_in(B, h, w))
    W64, W32 = cell_weights(params), cell_weights(params, torch.float32)
    c = {"T": T, "B": B, "h": h, "w": w, "x": x, "h0": h0, "c0": c0}
    c["fwd64"], c["fwd_e2"] = fwd_e2(W64, x, h0, c0)
    f32 = recur_fwd(W32, x, h0, c0)
    c["fwd_f32"] = {o: rel_err(f32[o], c["fwd64"][o]) for o in ("h", "c", "gates")}
    # the readout's cotangent of every h_t: the oracle's head on the fp32 recurrence's h_t
    S = ref_cpu.spatial_basis(h, w)
    Gl, Gv = (torch.from_numpy(detinit.cotangent(s, (T, B, 18))) for s in (2, 3))
    dO = []
    for t in range(T):
        O = f32["h"][t].clone().requires_grad_(True)
        lg, vl, _ = ref_cpu._head(P, O.transpose(1, 3), S, 4, None, None)
        (gO,) = torch.autograd.grad((lg * Gl[t]).sum() + (vl * Gv[t]).sum(), O)
        dO.append(gO)
    dO = torch.stack(dO)
    # the cotangents a following call hands over, at the scale of the readout's: every backward case has them
    dhT, dcT = (to_ref(t.reshape(B * h * w, 128), B, h, w) for t in state_cot(B, h, w, float(dO.abs().max())))
    args = _bwd_inputs(W32, x, h0, c0, dO, dhT, dcT)
    c["bwd64"], c["bwd_e2"] = bwd_e2(W64, *args, sites=sites)
    b32 = bptt(W32, *args)
    c["bwd_f32"] = {o: rel_err(b32[o], c["bwd64"][o]) for o in c["bwd64"]}
    return c


@functools.lru_cache(maxsize=None)
def cell_case(B, h, w):
    """The cell component entry's inputs, NHWC as the entry takes them, and the references on them."""
    M = B * h * w
    io = {"x": rnd((B, h, w, 64), 1, 3.0), "h0": rnd((B, h, w, 128), 2), "c0": rnd((B, h, w, 128), 3),
          "dh1": rnd((B, h, w, 128), 4), "dc1": rnd((B, h, w, 128), 5)}
    r = {k: to_ref(v.reshape(M, -1), B, h, w) for k, v in io.items()}
    W64, W32 = cell_weights(), cell_weights(dtype=torch.float32)
    c = {"B": B, "h": h, "w": w, "io": io, "ref_in": r}
    x = r["x"][None]
    c["fwd64"], c["fwd_e2"] = fwd_e2(W64, x, r["h0"], r["c0"])
    f32 = recur_fwd(W32, x, r["h0"], r["c0"])
    c["fwd_f32"] = {o: rel_err(f32[o], c["fwd64"][o]) for o in ("h", "c", "gates")}
    # one step: the entry's dh1 is the whole cotangent of h_1 (dO = 0).  The entry keeps its gates in a workspace
    # of its own layout, so forward + backward is the unit here: the reference backward reads the fp64 forward's
    # products, the fp32 stand-in (like a kernel) its own fp32 forward's
    rest = (r["h0"], r["c0"], torch.zeros(1, B, 128, w, h), r["dh1"], r["dc1"])
    c["bwd64"], c["bwd_e2"] = bwd_e2(W64, *_bwd_inputs(W64, x.double(), *rest))
    b32 = bptt(W32, *_bwd_inputs(W32, x, *rest))
    c["bwd_f32"] = {o: rel_err(b32[o], c["bwd64"][o]) for o in c["bwd64"]}
    return c


@functools.lru_cache(maxsize=None)
def cnn_case(N, H, W):
    """The vision CNN component entry's inputs (frames (N,H,W,3) scaled, dy2 (N,h,w,64) NHWC) and the
    references on them."""
    h, w = ref_cpu.grid_of(H, W)
    X = frames(1, N, H, W, FRAME_SCALE)[0]
    dy2 = rnd((N, h, w, 64), 6)
    x_ref, dy2_ref = X.permute(0, 3, 2, 1).contiguous(), dy2.permute(0, 3, 2, 1).contiguous()
    W64, W32 = cnn_weights(), cnn_weights(dtype=torch.float32)
    c = {"N": N, "h": h, "w": w, "X": X, "dy2": dy2, "x_ref": x_ref, "dy2_ref": dy2_ref}
    c["ref64"], c["e2"] = cnn_e2(W64, x_ref, dy2_ref)
    f32 = cnn_pieces(W32, x_ref, dy2_ref)
    c["f32"] = {o: rel_err(f32[o], c["ref64"][o]) for o in c["ref64"]}
    return c
