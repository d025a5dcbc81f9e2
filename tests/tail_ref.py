"""fp64 statement of the policy tail (everything after the ConvLSTM), layer by
layer, with a per-element error bound for the kernels that compute it, and the
dispatch rule that picks those kernels restated in Python.

Reference: attention.py:184-198 (QueryNetwork), :277-282 / :350 (answer MLP),
:354-358 (policy_core LSTMCell, zero state and carried state), :365-367 (heads)
and their autograd backward.  Kernels: csrc/rt.h (tail_gemm, head_gemm,
k_skinny_gemm), csrc/rt_backward.hip (tail_dgrad, tail_wgrad), csrc/gemm.h
(gemm_kernel, gemm_mma_tile), csrc/epilogues.h.

Every layer function takes the reference's own parameter tensors (fp64; the
packed layouts k_W1p / k_Wihp / k_Wihhp / k_Whd and the gate interleave
4u + g are undone here, never read back) and that layer's input AS THE KERNEL
STORED IT (include/aaa.h AAA_WS_TAIL_*), and returns (out, S): the fp64 output
and S = sum_k |a_k| |b_k| (+ |bias|) per output element.

Dispatch (rt.h; restated in ``fwd_dispatch`` / ``dgrad_dispatch`` /
``wgrad_dispatch``)
  forward GEMMs (tail_gemm): Nj <= 8 columns, K % 4 == 0, both pitches % 4 == 0
      -> k_skinny_gemm<EP, 1> (Nj == 1) or <EP, 8>; else head_gemm.
  head_gemm: tiles = cdiv(Mi, 64) cdiv(Nj, 64) nsplit;  < 192 -> CFK4 (32x64,
      BK 64, 4 wave groups splitting each BK slab), else CF (64x64, BK 32).
  weight gradients: nsplit = min(max(1, 1024 // tiles), max(1, F // 256)); the
      launch rounds a slice to whole BK tiles of the tile it runs
      (kchunk = ceil(ceil(F / nsplit) / BK) BK, slices = ceil(F / kchunk)), the
      slices accumulate with atomics into a zeroed buffer.
  arithmetic: fp32 cfg -> S6 (AAA_F32_SPLIT6=0: the fp32 MFMA); bf16 cfg -> S3
      (AAA_TAIL_SPLIT3=0: the fp32 MFMA).  The skinny kernels are plain fp32
      FMAs in every cfg.

Bounds.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16: 8 significand bits, round to nearest).
|kernel - fp64| <= gamma S + (epilogue terms) per element, gamma = eps + n u:
eps the representation error of the arithmetic per product, n the length of
the longest chain of fp32 additions a product passes through (any summation
order of n + 1 terms is within n u sum|terms| to first order; the (1 + n u)
second-order factor is applied).

  fp32 MFMA (gemm_mma_tile, v_mfma_f32_32x32x2_f32): eps = u (each product
      rounded once at most).  A wave group owns every WK-th 16-k step of its K
      slice: kchunk / WK products enter one accumulator one after the other;
      then WK - 1 additions through LDS and at most ``slices`` atomic additions:
      n = ceil(kchunk / 16 / WK) 16 + (WK - 1) + slices.
  S3 (GemmCfgS3): a = ah + al + ea with |al| <= ub |a|, |ea| <= ub^2 |a|
      (al = bf16(a - ah), a - ah exact in fp32).  Accumulated: al bh + ah bl +
      ah bh, exact products of bf16 pairs.  Missing: al bl + ea b + a eb
      (- ea eb): eps = 3 ub^2 (1 + ub).  Three part products per k enter the
      accumulator: n = 3 ceil(kchunk / 16 / WK) 16 + (WK - 1) + slices, on
      terms whose magnitudes sum to at most (1 + 2 ub) |a| |b|.
  S6 (GemmCfgS6): a = ah + am + al + ea, |am| <= ub |a|, |al| <= ub^2 |a|,
      |ea| <= ub^3 |a|.  Accumulated: the six part products with i + j <= 2.
      Missing: am bl + al bm + al bl + ea b + a eb: eps = 4 ub^3 (1 + ub).
      n = 6 ceil(kchunk / 16 / WK) 16 + (WK - 1) + slices, magnitudes
      (1 + 2 ub + 3 ub^2) |a| |b|.
  skinny (k_skinny_gemm): a lane takes 4 k of every 256: per visit four
      products and four additions, ceil(K / 256) visits, then a 6-step
      butterfly: eps = u, n = 4 ceil(K / 256) + 6.

  A worst-case chain bound is loose by about sqrt(n) against what rounding
  really does, so a fault that loses ~2^-16 of each product (one of S6's three
  smallest kept products) hides inside n u at the tail's K; what these gates
  reject is shown by tests/test_tail_emulation.py.

Epilogues.  Bias add / store: 2 u |out|.  ReLU is 1-Lipschitz: the GEMM bound
carries over to the stored output, compared as a value (never as a mask).
Gates: sigm_acc = 1 / (1 + expf(-x)) and tanhf (ocml); their error is not
stated in a document this repository can cite, so it was measured
(TAU_MEASURED = 6.2e-8, DESIGN.md "Policy tail: accuracy") and enters as
TAU = 4 x measured = 2.5e-7 <= TAU_CAP = 1e-5 absolute: |gate - fp64| <= L (gamma S +
2 u |z|) + TAU with L = 1/4 (sigmoid) or 1 (tanh).  c and h are checked from
the stored gates: |c - (gf c' + gi gc)| <= 3 u (|gf c'| + |gi gc|), |h - go
tanh(c)| <= |go| TAU + 2 u |h|.  gate_bwd is linear in dh and dc: dz = dh A +
dc Bc with A, Bc products of stored gates and tanh(c); its bound is |A| e_dh +
|Bc| e_dc + 2 TAU (|dh| + e_dh) + 12 u (|dh A| + |dc Bc|).
Column sums (bias gradients) of n rows in any order: n u sum|x|.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24
UB = 2.0 ** -8
# worst |gate - fp64 gate| over the F = 33, (nq, A) = (4, 18) zero-state case on the fp32 MFMA (MI355X), measured
# by tests/test_gpu_tail.py (it prints the value); the bound uses 4 x this, capped.
TAU_MEASURED = 6.208e-8
TAU_CAP = 1e-5
TAU = min(4 * TAU_MEASURED, TAU_CAP)
assert TAU <= TAU_CAP

SKINNY_MAX = 8
TILES = {"CFK4": dict(BI=32, BJ=64, BK=64, WK=4), "CF": dict(BI=64, BJ=64, BK=32, WK=1)}
ARITH = ("f32", "S3", "S6")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ dispatch --
def head_tile(Mi, Nj, nsplit=1):
    """rt.h head_gemm, product build (AAA_HEAD_TILE = 0)."""
    return "CFK4" if cdiv(Mi, 64) * cdiv(Nj, 64) * max(nsplit, 1) < 192 else "CF"


def kslices(K, BK, nsplit):
    """gemm.h launch_gemm: (kchunk, slices run) for a requested nsplit."""
    kc = cdiv(cdiv(K, max(nsplit, 1)), BK) * BK
    return kc, cdiv(K, kc)


def wgrad_splits(tiles, K, BK=32):
    """rt.h wgrad_splits (tail_wgrad passes CF::BK whatever tile then runs)."""
    return min(max(1, 1024 // max(tiles, 1)), max(1, K // (8 * BK)))


def fwd_dispatch(Mi, Nj, K, lda, ldb):
    """-> (kernel, slices): rt.h tail_gemm."""
    if Nj <= SKINNY_MAX and K % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0:
        return ("skinny1" if Nj == 1 else "skinny8"), 1
    return head_tile(Mi, Nj), 1


def dgrad_dispatch(Mi, Nj, K):
    return head_tile(Mi, Nj), 1


def wgrad_dispatch(Mi, Nj, F):
    ns = wgrad_splits(cdiv(Mi, 64) * cdiv(Nj, 64), F)
    tile = head_tile(Mi, Nj, ns)
    return tile, kslices(F, TILES[tile]["BK"], ns)[1]


def dims(nq, A, stateful):
    qd, ans_in = 72 * nq, 256 * nq + 2
    return dict(nq=nq, A=A, qd=qd, ans_in=ans_in, ans_ld=(ans_in + 7) // 8 * 8, ldy=(2 * A + 3) // 4 * 4,
                da=(256 if stateful else 184) * nq)


def plan(nq, A, T, B, stateful):
    """Every tail GEMM launch of one forward and one HEAD backward, in launch order:
    {"fwd": [(layer, kernel, slices, K)], "bwd": [...]}."""
    d = dims(nq, A, stateful)
    F, qd, al, ldy, da = T * B, d["qd"], d["ans_ld"], d["ldy"], d["da"]
    fwd, bwd = [], []

    def f(layer, Mi, Nj, K, lda, ldb):
        fwd.append((layer,) + fwd_dispatch(Mi, Nj, K, lda, ldb) + (K,))

    def g(layer, Mi, Nj, K):
        bwd.append((layer,) + dgrad_dispatch(Mi, Nj, K) + (K,))

    def w(layer, Mi, Nj):
        bwd.append((layer,) + wgrad_dispatch(Mi, Nj, F) + (F,))

    if not stateful:
        f("answer0", 512, F, al, al, al)
        f("answer2", 256, F, 512, 512, 512)
        f("lstm", 1024, F, 256, 256, 256)
        f("heads", 2 * A, F, 256, 256, 256)
        w("heads.w", ldy, 256); g("heads.d", 256, F, ldy)
        w("lstm.w", 1024, 256); g("lstm.d", 256, F, 1024)
        w("answer2.w", 256, 512); g("answer2.d", 512, F, 256)
        w("answer0.w", 512, al); g("answer0.d", da, F, 512)
    else:
        for _ in range(T):
            f("query0", 128, B, 256, 256, 256)
            f("query2", qd, B, 128, 128, 128)
            f("query4", qd, B, qd, qd, qd)
            f("answer0", 512, B, al, al, al)
            f("answer2", 256, B, 512, 512, 512)
            f("lstm", 1024, B, 512, 512, 512)
        f("heads", 2 * A, F, 256, 256, 256)
        for _ in range(T):
            g("heads.d", 256, B, ldy); g("lstm.d", 512, B, 1024); g("answer2.d", 512, B, 256)
            g("answer0.d", da, B, 512); g("query4.d", qd, B, qd); g("query2.d", 128, B, qd); g("query0.d", 256, B, 128)
        w("heads.w", ldy, 256); w("lstm.w", 1024, 512); w("answer2.w", 256, 512); w("answer0.w", 512, al)
        w("query4.w", qd, qd); w("query2.w", qd, 128); w("query0.w", 128, 256)
    return {"fwd": fwd, "bwd": bwd}


def token(kernel, arith, slices=1):
    """One launch as the timers' variant names it (rt_core.hip tail_ran)."""
    s = kernel if kernel.startswith("skinny") else f"{kernel}/{arith}"
    return s + (f" x{slices}" if slices > 1 else "")


def variant_log(launches, arith):
    """The launches as aaa_timing_stats renders them: equal neighbours counted."""
    out = []
    for _, kernel, slices, _ in launches:
        t = token(kernel, arith, slices)
        if out and out[-1][0] == t:
            out[-1][1] += 1
        else:
            out.append([t, 1])
    return ", ".join(t + (f"*{n}" if n > 1 else "") for t, n in out)


# -------------------------------------------------------------------- bounds --
def gamma(kernel, arith, K, slices=1):
    """gamma of the module docstring for one launch with reduction length K."""
    if kernel.startswith("skinny"):
        n = 4 * cdiv(K, 256) + 6
        return (U + n * U) * (1 + n * U)
    t = TILES[kernel]
    kc = kslices(K, t["BK"], slices)[0] if slices > 1 else cdiv(K, t["BK"]) * t["BK"]
    steps = cdiv(cdiv(min(kc, K), 16), t["WK"]) * 16   # k values of the longest wave group's share
    tail = (t["WK"] - 1) + slices
    if arith == "f32":
        eps, n, mag = U, steps + tail, 1.0
    elif arith == "S3":
        eps, n, mag = 3 * UB ** 2 * (1 + UB), 3 * steps + tail, 1 + 2 * UB
    else:
        eps, n, mag = 4 * UB ** 3 * (1 + UB), 6 * steps + tail, 1 + 2 * UB + 3 * UB ** 2
    return eps + n * U * mag * (1 + n * U)


def gemm_bound(out, S, g):
    """gamma S plus the epilogue's bias add and store."""
    return g * S + 2 * U * out.abs()


# -------------------------------------------------------------------- layers --
def lin(W, x, bias=None):
    """x (N, K) @ W (Mi, K)^T (+ bias): (out, S), fp64."""
    W, x = W.double(), x.double()
    out, S = x @ W.T, x.abs() @ W.abs().T
    if bias is not None:
        out, S = out + bias.double(), S + bias.double().abs()
    return out, S


def relu(o_S):
    return o_S[0].clamp_min(0), o_S[1]


def interleave(z):
    """(N, 4*256) in the reference's gate-major order g*256 + u -> the kernels' 4u + g."""
    return z.reshape(z.shape[0], 4, 256).transpose(1, 2).reshape(z.shape[0], 1024)


def deinterleave(z):
    return z.reshape(z.shape[0], 256, 4).transpose(1, 2).reshape(z.shape[0], 1024)


def query0(P, h): return relu(lin(P["query.model.0.weight"], h, P["query.model.0.bias"]))
def query2(P, q1): return relu(lin(P["query.model.2.weight"], q1, P["query.model.2.bias"]))
def query4(P, q2): return lin(P["query.model.4.weight"], q2, P["query.model.4.bias"])


def answer0(P, ans):
    """ans: the stored (F, ans_ld) rows; the padding columns multiply packed zeros."""
    W = P["answer_processor.0.weight"]
    return relu(lin(W, ans[:, :W.shape[1]], P["answer_processor.0.bias"]))


def answer2(P, hid): return lin(P["answer_processor.2.weight"], hid, P["answer_processor.2.bias"])


def lstm_pre(P, x, stateful):
    """Gate pre-activations, interleaved (4u + g): W_ih x (+ W_hh h for the [answer | h] rows) + b_ih + b_hh."""
    W = P["policy_core.weight_ih"]
    if stateful:
        W = torch.cat([W, P["policy_core.weight_hh"]], 1)
    z, S = lin(W, x, P["policy_core.bias_ih"].double() + P["policy_core.bias_hh"].double())
    return interleave(z), interleave(S)


def gates_of(z):
    """(N, 1024) interleaved pre-activations -> activations (i, f, c~, o), fp64, and their Lipschitz constants."""
    z4 = z.reshape(z.shape[0], 256, 4)
    g = torch.stack([torch.sigmoid(z4[..., 0]), torch.sigmoid(z4[..., 1]), torch.tanh(z4[..., 2]),
                     torch.sigmoid(z4[..., 3])], -1)
    L = torch.tensor([0.25, 0.25, 1.0, 0.25], dtype=torch.float64).expand_as(g)
    return g.reshape(z.shape[0], 1024), L.reshape(z.shape[0], 1024)


def gate_bound(z, S, g):
    L = gates_of(z)[1]
    return L * (g * S + 2 * U * z.abs()) + TAU


def cell_from_gates(gates, cprev=None):
    """c, h and their bounds from the STORED gates (N, 1024) (and c_{t-1})."""
    g4 = gates.double().reshape(gates.shape[0], 256, 4)
    gi, gf, gc, go = g4.unbind(-1)
    a = gf * (cprev.double() if cprev is not None else 0.0)
    b = gi * gc
    c = a + b
    return c, 3 * U * (a.abs() + b.abs())


def h_from(gates, c):
    go = gates.double().reshape(gates.shape[0], 256, 4)[..., 3]
    h = go * torch.tanh(c.double())
    return h, go.abs() * TAU + 2 * U * h.abs()


def heads(P, h):
    W = torch.cat([P["policy_head.0.weight"], P["values_head.0.weight"]])
    b = torch.cat([P["policy_head.0.bias"], P["values_head.0.bias"]])
    return lin(W, h, b)


# backward: dgrads (D = dY W), each on the cotangent the kernel stored
def heads_dgrad(P, dY, A):
    W = torch.cat([P["policy_head.0.weight"], P["values_head.0.weight"]])   # (2A, 256)
    return lin(W.T, dY[:, :2 * A])


def cell_bwd(dh, e_dh, gates, c, cprev=None, dc=None, e_dc=None):
    """csrc/epilogues.h gate_bwd in fp64 from the stored gates, c_t (and c_{t-1}, the carried dc): the gate
    pre-activations' cotangent (N, 1024) interleaved, its bound, the dc carry for t-1 and that carry's bound."""
    g4 = gates.double().reshape(gates.shape[0], 256, 4)
    gi, gf, gc, go = g4.unbind(-1)
    tc = torch.tanh(c.double())
    cp = cprev.double() if cprev is not None else torch.zeros_like(tc)
    dcin = dc.double() if dc is not None else torch.zeros_like(tc)
    edc = e_dc if e_dc is not None else torch.zeros_like(tc)
    k = go * (1 - tc * tc)                      # d dcc / d dh
    dcc = dcin + dh * k
    Bc = torch.stack([gc * (1 - gi) * gi, cp * (1 - gf) * gf, gi * (1 - gc * gc), torch.zeros_like(gi)], -1)
    A = Bc * k[..., None]
    A[..., 3] = tc * (1 - go) * go
    dz = dh[..., None] * A + dcin[..., None] * Bc
    bound = (A.abs() * e_dh[..., None] + Bc.abs() * edc[..., None] + 2 * TAU * (dh.abs() + e_dh)[..., None]
             + 12 * U * ((dh[..., None] * A).abs() + (dcin[..., None] * Bc).abs()))
    carry = dcc * gf
    e_carry = gf.abs() * (edc + k.abs() * e_dh + 2 * TAU * (dh.abs() + e_dh)) + 6 * U * (dcin.abs() + (dh * k).abs())
    n = gates.shape[0]
    return dz.reshape(n, 1024), bound.reshape(n, 1024), carry, e_carry


def lstm_dgrad(P, dLG, stateful):
    """[d answer | d h (recurrent)] = dgates [W_ih | W_hh]."""
    W = P["policy_core.weight_ih"]
    if stateful:
        W = torch.cat([W, P["policy_core.weight_hh"]], 1)
    return lin(W.T, deinterleave(dLG.double()))


def answer2_dgrad(P, dAO, hid):
    o, S = lin(P["answer_processor.2.weight"].T, dAO)
    m = (hid > 0).double()
    return o * m, S * m


def answer0_dgrad(P, dH1, da): return lin(P["answer_processor.0.weight"][:, :da].T, dH1)
def query4_dgrad(P, dQ, q2): return _masked(lin(P["query.model.4.weight"].T, dQ), q2)
def query2_dgrad(P, dq2, q1): return _masked(lin(P["query.model.2.weight"].T, dq2), q1)
def query0_dgrad(P, dq1): return lin(P["query.model.0.weight"].T, dq1)


def _masked(o_S, saved):
    m = (saved > 0).double()
    return o_S[0] * m, o_S[1] * m


def wgrad(dA, X):
    """out[i][j] = sum_f dA[f][i] X[f][j]: (out, S)."""
    dA, X = dA.double(), X.double()
    return dA.T @ X, dA.abs().T @ X.abs()


def colsum(x):
    """Bias gradient: (sum, bound) of the stored cotangent's columns."""
    x = x.double()
    return x.sum(0), x.shape[0] * U * x.abs().sum(0)


# --------------------------------------------------------------------- cases --
NQA = ((4, 18), (8, 5))


def _first(pred, lo=1, hi=4096):
    return next(F for F in range(lo, hi) if pred(F))


F_LSTM_CF = _first(lambda F: head_tile(1024, F) == "CF")                     # 705
F_ANSWER0_CF = _first(lambda F: head_tile(512, F) == "CF")                   # 1473
F_LSTM_WGRAD_CF = _first(lambda F: wgrad_dispatch(1024, 256, F)[0] == "CF")  # 768: CFK4 x2 -> CF x3
assert (F_LSTM_CF, F_ANSWER0_CF, F_LSTM_WGRAD_CF) == (705, 1473, 768)
assert wgrad_dispatch(1024, 256, 640) == ("CFK4", 2) and wgrad_dispatch(1024, 256, 768) == ("CF", 3)
ZERO_F = (1, 2, 8, 9, 33, 257, 520, F_LSTM_CF, F_LSTM_WGRAD_CF, F_ANSWER0_CF)
STATE_T, STATE_B = 3, (1, 3, 8, 9, 40)
# (nq, A, T, B, stateful): the zero-state cases as one step of F frames
CASES = [(nq, A, 1, F, False) for nq, A in NQA for F in ZERO_F] + \
        [(nq, A, STATE_T, B, True) for nq, A in NQA for B in STATE_B]


def case_id(c):
    return "nq{}A{}_T{}B{}{}".format(*c[:4], "_state" if c[4] else "")


def reachable():
    """Every (kernel, arithmetic) pair the product build can run in the tail."""
    return {(k, a) for k in ("CFK4", "CF") for a in ARITH} | {("skinny1", None), ("skinny8", None)}


def covered(cases=CASES):
    got = set()
    for nq, A, T, B, sc in cases:
        p = plan(nq, A, T, B, sc)
        for _, kernel, _, _ in p["fwd"] + p["bwd"]:
            got |= {(kernel, None)} if kernel.startswith("skinny") else {(kernel, a) for a in ARITH}
    return got


assert covered() == reachable(), reachable() - covered()
# the boundaries the cases are there for: both skinny kernels and the first size past them, CFK4 under the
# stateful epilogues, slice counts 1, 2, 3 and 5 and both tiles among the weight gradients
assert {plan(4, 18, STATE_T, B, True)["fwd"][5][1] for B in STATE_B} == {"skinny1", "skinny8", "CFK4"}
assert {s for c in CASES for _, _, s, _ in plan(*c)["bwd"]} >= {1, 2, 3, 5}


def dispatch_table():
    """DESIGN.md "Policy tail: dispatch": layer x F range -> kernel and K slices, zero-state core, (nq, A) = (4, 18)."""
    rows, top = [], max(ZERO_F)
    edges = sorted({1} | {F for F in range(2, top + 1) if [x[1:3] for x in _zero_plan(F)] != [x[1:3] for x in _zero_plan(F - 1)]})
    for lo, hi in zip(edges, edges[1:] + [top + 1]):
        rows.append((lo, hi - 1, [(x[0], token(x[1], "A", x[2])) for x in _zero_plan(lo)]))
    return rows


def dispatch_markdown():
    """The table as DESIGN.md holds it (tests/test_tail_emulation.py compares the two)."""
    rows = dispatch_table()
    layers = [layer for layer, _ in rows[0][2]]
    out = ["| F | " + " | ".join(layers) + " |", "|---|" + "---|" * len(layers)]
    for lo, hi, cells in rows:
        out.append(f"| {lo}" + (f"–{hi}" if hi > lo else "") + " | " + " | ".join(t.replace("/A", "") for _, t in cells) + " |")
    return "\n".join(out)


def _zero_plan(F):
    p = plan(4, 18, 1, F, False)
    return p["fwd"] + p["bwd"]


# ----------------------------------------------------------------- emulation --
def _cut(x, parts):
    """fp32 x -> its first ``parts`` bf16 parts (gemm.h split_bf16 / split3_bf16), as fp32 tensors."""
    out, r = [], x.float()
    for _ in range(parts):
        p = r.bfloat16().float()
        out.append(p)
        r = r - p
    return out


def emulate_gemm(a, b, kernel, arith, slices=1, fault=None):
    """D[i][j] = sum_k a[i][k] b[j][k] in float32 the way ``kernel`` orders it: 16-k steps dealt to WK wave
    groups, summed through "LDS", K slices added one after the other; S3 / S6 on real bf16 cuts in the kernel's
    product order.  ``fault``: "ragged" (the last, partial 16-k step lost), "cross" (S3: lo.hi lost, S6: mid.hi
    lost), "frames256" (the K loop stops at K - K % 256: a weight gradient's last frames lost)."""
    a, b = a.float(), b.float()
    K = a.shape[1]
    if fault == "frames256":
        K -= K % 256
    if kernel.startswith("skinny"):
        acc = torch.zeros(a.shape[0], b.shape[0], 64)
        for k0 in range(0, K, 256):
            for lane in range(min(64, cdiv(K - k0, 4))):
                k = k0 + 4 * lane
                acc[:, :, lane] += (a[:, None, k:k + 4] * b[None, :, k:k + 4]).sum(-1)
        n = 64
        while n > 1:
            n //= 2
            acc = acc[:, :, :n] + acc[:, :, n:2 * n]
        return acc[:, :, 0]
    t = TILES[kernel]
    kc = kslices(K, t["BK"], slices)[0] if K else 0
    if arith == "f32":
        pa, pb, order = [a], [b], [(0, 0)]
    elif arith == "S3":
        pa, pb, order = _cut(a, 2), _cut(b, 2), [(1, 0), (0, 1), (0, 0)]
        if fault == "cross":
            order = [(0, 1), (0, 0)]
    else:
        pa, pb, order = _cut(a, 3), _cut(b, 3), [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]
        if fault == "cross":
            order.remove((1, 0))
    D = torch.zeros(a.shape[0], b.shape[0])
    for kb in range(0, K, max(kc, 1)):
        ke = min(K, kb + kc)
        accs = [torch.zeros_like(D) for _ in range(t["WK"])]
        for s, k in enumerate(range(kb, ke, 16)):
            if fault == "ragged" and ke - k < 16:
                continue
            acc = accs[(s % (t["BK"] // 16)) % t["WK"]]
            for i, j in order:
                acc += pa[i][:, k:min(k + 16, ke)] @ pb[j][:, k:min(k + 16, ke)].T
        part = accs[0]
        for w in accs[1:]:
            part = part + w
        D = D + part
    return D


# -------------------------------------------------------------------- checks --
# One run of a case as a dict ``o`` (tests/test_gpu_tail.py fills it from the workspace regions of a GPU run,
# ``emulate`` below from float32 arithmetic on the CPU): "P" fp64 parameters, "g" name -> gradient, the stored
# layer inputs / outputs.  check_zero_state / check_stateful hold every layer of it to its bound.
class Check:
    """Collects |got - ref| <= bound over every element of every layer; prints each layer's worst ratio."""

    def __init__(self, what):
        self.what, self.bad, self.worst = what, [], {}

    def __call__(self, layer, got, ref, bound):
        got, ref = got.double().reshape(ref.shape), ref.double()
        err = (got - ref).abs()
        ok = torch.isfinite(got).all() and bool((err <= bound).all())
        ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() and torch.isfinite(got).all() else math.inf
        self.worst[layer] = max(self.worst.get(layer, 0.0), ratio)
        if not ok:
            i = int((err - bound).nan_to_num(math.inf).argmax())
            self.bad.append(f"{layer}: err/bound {ratio:.3g} (err {float(err.reshape(-1)[i]):.3e}, bound "
                            f"{float(bound.reshape(-1)[i]):.3e}, ref {float(ref.reshape(-1)[i]):.3e})")

    def exact(self, layer, got, ref):
        if not torch.equal(got.reshape(ref.shape), ref):
            self.bad.append(f"{layer}: not bit-identical")

    def report(self):
        return f"[tail] {self.what}: " + " ".join(f"{k} {v:.3f}" for k, v in self.worst.items())


def gammas(plan_, arith):
    """layer -> gamma of its launch (the stateful core's per-step launches of one layer are alike)."""
    return {layer: gamma(kernel, arith, K, slices) for layer, kernel, slices, K in plan_["fwd"] + plan_["bwd"]}


def _bias_bound(ref, b):
    return b + 2 * U * ref.abs()


def _check_common(ck, o, G, A, d, h_heads):
    """What both cores share: answer.0, the heads, dY, answer.0's dgrad, their weight and bias gradients."""
    P = o["P"]
    if float(o["ans"][:, d["ans_in"]:].abs().max()) != 0.0:
        ck.bad.append("ans: padding columns not zero")
    ref, S = answer0(P, o["ans"])
    ck("answer0", o["hid"], ref, gemm_bound(ref, S, G["answer0"]))
    ref, S = heads(P, h_heads)
    ck("heads", torch.cat([o["logits"], o["values"]], 1), ref, gemm_bound(ref, S, G["heads"]))
    dY = o["dY"]
    ck.exact("dY", dY[:, :2 * A], torch.cat([o["Gl"], o["Gv"]], 1))
    if dY.shape[1] > 2 * A and float(dY[:, 2 * A:].abs().max()) != 0.0:
        ck.bad.append("dY: padding columns not zero")
    ref, S = answer0_dgrad(P, o["dhid"], d["da"])
    ck("answer0.d", o["dans"], ref, gemm_bound(ref, S, G["answer0.d"]))
    for name, dA, X, layer in (("policy_head.0", dY[:, :A], h_heads, "heads.w"),
                               ("values_head.0", dY[:, A:2 * A], h_heads, "heads.w"),
                               ("answer_processor.0", o["dhid"], o["ans"][:, :d["ans_in"]], "answer0.w")):
        ref, S = wgrad(dA, X)
        ck(layer, o["g"][name + ".weight"], ref, gemm_bound(ref, S, G[layer]))
        ck(name + ".bias", o["g"][name + ".bias"], *_colsum_bound(dA))


def _colsum_bound(x):
    ref, b = colsum(x)
    return ref, _bias_bound(ref, b)


def check_zero_state(o, case, arith):
    nq, A, T, B, _ = case
    P, d = o["P"], dims(nq, A, False)
    G = gammas(plan(*case), arith)
    ck = Check(f"{case_id(case)} {arith}")
    _check_common(ck, o, G, A, d, o["h"])
    ref, S = answer2(P, o["hid"])
    ck("answer2", o["ao"], ref, gemm_bound(ref, S, G["answer2"]))
    z, S = lstm_pre(P, o["ao"], False)
    ck("lstm.gates", o["gates"], gates_of(z)[0], gate_bound(z, S, G["lstm"]))
    ck("lstm.c", o["c"], *cell_from_gates(o["gates"]))
    ck("lstm.h", o["h"], *h_from(o["gates"], o["c"]))
    dh, S = heads_dgrad(P, o["dY"], A)
    dz, b, _, _ = cell_bwd(dh, G["heads.d"] * S, o["gates"], o["c"])
    ck("heads.d+cell", o["dgates"], dz, b)
    ref, S = lstm_dgrad(P, o["dgates"], False)
    ck("lstm.d", o["dao"], ref, gemm_bound(ref, S, G["lstm.d"]))
    ref, S = answer2_dgrad(P, o["dao"], o["hid"])
    ck("answer2.d", o["dhid"], ref, gemm_bound(ref, S, G["answer2.d"]))
    ref, S = wgrad(deinterleave(o["dgates"]), o["ao"])
    ck("lstm.w", o["g"]["policy_core.weight_ih"], ref, gemm_bound(ref, S, G["lstm.w"]))
    if float(o["g"]["policy_core.weight_hh"].abs().max()) != 0.0:
        ck.bad.append("policy_core.weight_hh: gradient not exactly 0")
    for nm in ("policy_core.bias_ih", "policy_core.bias_hh"):
        ck(nm, o["g"][nm], *_colsum_bound(deinterleave(o["dgates"])))
    ref, S = wgrad(o["dao"], o["hid"])
    ck("answer2.w", o["g"]["answer_processor.2.weight"], ref, gemm_bound(ref, S, G["answer2.w"]))
    ck("answer_processor.2.bias", o["g"]["answer_processor.2.bias"], *_colsum_bound(o["dao"]))
    return ck


def check_stateful(o, case, arith):
    nq, A, T, B, _ = case
    F = T * B
    P, d = o["P"], dims(nq, A, True)
    G = gammas(plan(*case), arith)
    ck = Check(f"{case_id(case)} {arith}")
    ch, cc = o["ch"], o["cc"]
    hprev, cprev, hnext, cnext = (t.reshape(F, 256) for t in (ch[:-1], cc[:-1], ch[1:], cc[1:]))
    _check_common(ck, o, G, A, d, hnext)
    ck.exact("core_h0", ch[0], o["core_h0"])
    ck.exact("core_c0", cc[0], o["core_c0"])
    ck.exact("core_hT", o["core_hT"], ch[T])
    ck.exact("core_cT", o["core_cT"], cc[T])
    ck.exact("aox.h", o["aox"][:, 256:], hprev)
    ref, S = query0(P, hprev)
    ck("query0", o["q1"], ref, gemm_bound(ref, S, G["query0"]))
    ref, S = query2(P, o["q1"])
    ck("query2", o["q2"], ref, gemm_bound(ref, S, G["query2"]))
    ref, S = query4(P, o["q2"])
    ck("query4", o["q"], ref, gemm_bound(ref, S, G["query4"]))
    ref, S = answer2(P, o["hid"])
    ck("answer2", o["aox"][:, :256], ref, gemm_bound(ref, S, G["answer2"]))
    z, S = lstm_pre(P, o["aox"], True)
    ck("lstm.gates", o["gates"], gates_of(z)[0], gate_bound(z, S, G["lstm"]))
    ck("lstm.c", cnext, *cell_from_gates(o["gates"], cprev))
    ck("lstm.h", hnext, *h_from(o["gates"], cnext))
    # backward: the dh carry entering step t is step t+1's EpiStoreAddT sum, evaluated from its two stored parts;
    # the dc carry free-runs in fp64 from dcore_cT with its bound carried along (neither carry is stored)
    rows = lambda x, t: x[t * B:(t + 1) * B]   # noqa: E731
    q0d, q0S = query0_dgrad(P, o["dq1"])
    dh_in = q0d + o["daox"][:, 256:].double()
    e_in = G["query0.d"] * q0S + 2 * U * dh_in.abs()
    dc, e_dc = o["dcore_cT"].double(), torch.zeros(B, 256, dtype=torch.float64)
    dhT = o["dcore_hT"].double()
    dhg, dhS = heads_dgrad(P, o["dY"], A)
    for t in range(T - 1, -1, -1):
        carry, e_c = (dhT, torch.zeros_like(dhT)) if t == T - 1 else (rows(dh_in, t + 1), rows(e_in, t + 1))
        dh = rows(dhg, t) + carry
        e_dh = G["heads.d"] * rows(dhS, t) + e_c + 2 * U * dh.abs()
        dz, b, dc, e_dc = cell_bwd(dh, e_dh, rows(o["gates"], t), cc[t + 1], cc[t], dc, e_dc)
        ck("heads.d+cellS", rows(o["dgates"], t), dz, b)
    ck("dcore_c0", o["dcore_c0"], dc, e_dc + 2 * U * dc.abs())
    ck("dcore_h0", o["dcore_h0"], rows(dh_in, 0), rows(e_in, 0))
    ref, S = lstm_dgrad(P, o["dgates"], True)
    ck("lstm.d", o["daox"], ref, gemm_bound(ref, S, G["lstm.d"]))
    ref, S = answer2_dgrad(P, o["daox"][:, :256], o["hid"])
    ck("answer2.d", o["dhid"], ref, gemm_bound(ref, S, G["answer2.d"]))
    ref, S = query4_dgrad(P, o["dq"], o["q2"])
    ck("query4.d", o["dq2"], ref, gemm_bound(ref, S, G["query4.d"]))
    ref, S = query2_dgrad(P, o["dq2"], o["q1"])
    ck("query2.d", o["dq1"], ref, gemm_bound(ref, S, G["query2.d"]))
    ref, S = wgrad(deinterleave(o["dgates"]), o["aox"])
    ck("lstm.w", torch.cat([o["g"]["policy_core.weight_ih"].reshape(1024, 256),
                            o["g"]["policy_core.weight_hh"].reshape(1024, 256)], 1), ref, gemm_bound(ref, S, G["lstm.w"]))
    for nm in ("policy_core.bias_ih", "policy_core.bias_hh"):
        ck(nm, o["g"][nm], *_colsum_bound(deinterleave(o["dgates"])))
    for name, dA, X, layer in (("answer_processor.2", o["daox"][:, :256], o["hid"], "answer2.w"),
                               ("query.model.4", o["dq"], o["q2"], "query4.w"),
                               ("query.model.2", o["dq2"], o["q1"], "query2.w"),
                               ("query.model.0", o["dq1"], hprev, "query0.w")):
        ref, S = wgrad(dA, X)
        ck(layer, o["g"][name + ".weight"], ref, gemm_bound(ref, S, G[layer]))
        ck(name + ".bias", o["g"][name + ".bias"], *_colsum_bound(dA))
    return ck


def check(o, case, arith):
    return check_stateful(o, case, arith) if case[4] else check_zero_state(o, case, arith)


# ---------------------------------------------- emulated runs (CPU, float32) --
FAULTS = ("ragged", "cross", "bias_per_slice", "relu_row", "frames256", "pitch256")


def _rnd(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).float()


def _gate_bwd32(dh, gates, c, cprev, dc):
    """epilogues.h gate_bwd in float32."""
    gi, gf, gc, go = gates.reshape(gates.shape[0], 256, 4).unbind(-1)
    tc = torch.tanh(c)
    dcc = dc + dh * go * (1 - tc * tc)
    dz = torch.stack([dcc * gc * (1 - gi) * gi, dcc * cprev * (1 - gf) * gf, dcc * gi * (1 - gc * gc),
                      dh * tc * (1 - go) * go], -1)
    return dz.reshape(gates.shape[0], 1024), dcc * gf


def emulate(P, case, arith, fault=None):
    """The run dict ``o`` of ``check`` from float32 arithmetic on the CPU: every tail GEMM through emulate_gemm on
    the kernel and slice count the dispatch gives it, the epilogues in float32, on seeded answer rows, cotangents
    and state (the attention readout between the layers is not part of the tail: its products are seeded).
    ``fault`` seeds one of FAULTS into every launch it applies to."""
    nq, A, T, B, sc = case
    F, d = T * B, dims(nq, A, sc)
    pl = plan(*case)
    disp = {layer: (kernel, slices) for layer, kernel, slices, _ in pl["fwd"] + pl["bwd"]}
    W = {k: v.float() for k, v in P.items()}

    def gemm(layer, a, b, bias=None, act=False, mask=None):
        """(Nj, Mi) = b a^T (+ bias) through ``layer``'s kernel; act: ReLU; mask: ReLU backward by a saved output."""
        kernel, slices = disp[layer]
        f = fault if fault in ("ragged", "cross") or (fault == "frames256" and layer.endswith(".w")) else None
        out = emulate_gemm(a, b, kernel, arith, slices, f).T
        if bias is not None:
            out = out + bias * (TILES[kernel]["WK"] if fault == "bias_per_slice" and kernel in TILES else 1)
        if act:
            sign = out
            if fault == "relu_row":   # rows 31, 63, ... of the D tile take the next row's sign
                sign = out.clone()
                idx = torch.arange(31, out.shape[1] - 1, 32)
                sign[:, idx] = out[:, idx + 1]
            out = torch.where(sign > 0, out, torch.zeros_like(out))
        if mask is not None:
            out = torch.where(mask > 0, out, torch.zeros_like(out))
        return out.contiguous()

    a0w = torch.zeros(512, d["ans_ld"]); a0w[:, :d["ans_in"]] = W["answer_processor.0.weight"]
    wih = interleave(W["policy_core.weight_ih"].T).T.contiguous()      # rows 4u + g
    whh = interleave(W["policy_core.weight_hh"].T).T.contiguous()
    blc = interleave((W["policy_core.bias_ih"] + W["policy_core.bias_hh"])[None])[0]
    whd = torch.zeros(d["ldy"], 256)
    whd[:2 * A] = torch.cat([W["policy_head.0.weight"], W["values_head.0.weight"]])
    bhd = torch.cat([W["policy_head.0.bias"], W["values_head.0.bias"]])
    ans = torch.zeros(F, d["ans_ld"]); ans[:, :d["ans_in"]] = _rnd(11, (F, d["ans_in"]))
    Gl, Gv = _rnd(2, (F, A)), _rnd(3, (F, A))
    dY = torch.zeros(F, d["ldy"]); dY[:, :2 * A] = torch.cat([Gl, Gv], 1)
    o = {"P": P, "ans": ans, "Gl": Gl, "Gv": Gv, "dY": dY, "g": {}}
    g = o["g"]

    def act_gates(z):
        z4 = z.reshape(z.shape[0], 256, 4)
        return torch.stack([torch.sigmoid(z4[..., 0]), torch.sigmoid(z4[..., 1]), torch.tanh(z4[..., 2]),
                            torch.sigmoid(z4[..., 3])], -1).reshape(z.shape[0], 1024)

    def wg(layer, dA, X):
        return gemm(layer, dA.T.contiguous(), X.T.contiguous()).T.contiguous()

    def head_grads(h_heads):
        gw = wg("heads.w", dY, h_heads)
        g["policy_head.0.weight"], g["values_head.0.weight"] = gw[:A], gw[A:2 * A]
        g["policy_head.0.bias"], g["values_head.0.bias"] = dY[:, :A].sum(0), dY[:, A:2 * A].sum(0)

    if not sc:
        o["hid"] = gemm("answer0", a0w, ans, W["answer_processor.0.bias"], act=True)
        o["ao"] = gemm("answer2", W["answer_processor.2.weight"], o["hid"], W["answer_processor.2.bias"])
        o["gates"] = act_gates(gemm("lstm", wih, o["ao"], blc))
        gi, gf, gc, go = o["gates"].reshape(F, 256, 4).unbind(-1)
        o["c"] = gi * gc
        o["h"] = go * torch.tanh(o["c"])
        lv = gemm("heads", whd[:2 * A], o["h"], bhd)
        o["logits"], o["values"] = lv[:, :A].contiguous(), lv[:, A:].contiguous()
        head_grads(o["h"])
        dh = gemm("heads.d", whd.T.contiguous(), dY)
        o["dgates"], _ = _gate_bwd32(dh, o["gates"], o["c"], torch.zeros_like(dh), torch.zeros_like(dh))
        g["policy_core.weight_ih"] = deinterleave(wg("lstm.w", o["dgates"], o["ao"]).T).T
        g["policy_core.weight_hh"] = torch.zeros(1024, 256)
        g["policy_core.bias_ih"] = g["policy_core.bias_hh"] = deinterleave(o["dgates"]).sum(0)
        o["dao"] = gemm("lstm.d", wih.T.contiguous(), o["dgates"])
        g["answer_processor.2.weight"], g["answer_processor.2.bias"] = wg("answer2.w", o["dao"], o["hid"]), o["dao"].sum(0)
        o["dhid"] = gemm("answer2.d", W["answer_processor.2.weight"].T.contiguous(), o["dao"], mask=o["hid"])
        g["answer_processor.0.weight"] = wg("answer0.w", o["dhid"], ans)[:, :d["ans_in"]]
        g["answer_processor.0.bias"] = o["dhid"].sum(0)
        o["dans"] = gemm("answer0.d", a0w[:, :d["da"]].T.contiguous(), o["dhid"])
        return o

    wx = torch.cat([wih, whh], 1)
    qd = d["qd"]
    ch, cc = torch.zeros(T + 1, B, 256), torch.zeros(T + 1, B, 256)
    ch[0], cc[0] = _rnd(6, (B, 256), 0.5), _rnd(7, (B, 256), 0.5)
    z = lambda *s: torch.zeros(*s)   # noqa: E731
    o.update(core_h0=ch[0].clone(), core_c0=cc[0].clone(), q1=z(F, 128), q2=z(F, qd), q=z(F, qd), hid=z(F, 512),
             aox=z(F, 512), gates=z(F, 1024), dgates=z(F, 1024), daox=z(F, 512), dhid=z(F, 512), dans=z(F, d["da"]),
             dq=_rnd(12, (F, qd), 0.1), dq2=z(F, qd), dq1=z(F, 128), ch=ch, cc=cc)
    for t in range(T):
        r = slice(t * B, (t + 1) * B)
        o["q1"][r] = gemm("query0", W["query.model.0.weight"], ch[t], W["query.model.0.bias"], act=True)
        o["q2"][r] = gemm("query2", W["query.model.2.weight"], o["q1"][r], W["query.model.2.bias"], act=True)
        o["q"][r] = gemm("query4", W["query.model.4.weight"], o["q2"][r], W["query.model.4.bias"])
        o["hid"][r] = gemm("answer0", a0w, ans[r], W["answer_processor.0.bias"], act=True)
        o["aox"][r, :256] = gemm("answer2", W["answer_processor.2.weight"], o["hid"][r], W["answer_processor.2.bias"])
        o["aox"][r, 256:] = ch[t]
        x = o["aox"][r]
        if fault == "pitch256":   # row j of the operand read at j * 256 instead of j * 512
            flat = torch.cat([o["aox"][r].reshape(-1), torch.zeros(512)])
            x = torch.stack([flat[j * 256:j * 256 + 512] for j in range(B)])
        o["gates"][r] = act_gates(gemm("lstm", wx, x, blc))
        gi, gf, gc, go = o["gates"][r].reshape(B, 256, 4).unbind(-1)
        cc[t + 1] = gf * cc[t] + gi * gc
        ch[t + 1] = go * torch.tanh(cc[t + 1])
    o["core_hT"], o["core_cT"] = ch[T].clone(), cc[T].clone()
    hnext = ch[1:].reshape(F, 256)
    lv = gemm("heads", whd[:2 * A], hnext, bhd)
    o["logits"], o["values"] = lv[:, :A].contiguous(), lv[:, A:].contiguous()
    o["dcore_hT"], o["dcore_cT"] = _rnd(8, (B, 256), 0.1), _rnd(9, (B, 256), 0.1)
    dhc, dcc = o["dcore_hT"].clone(), o["dcore_cT"].clone()
    for t in range(T - 1, -1, -1):
        r = slice(t * B, (t + 1) * B)
        dh = gemm("heads.d", whd.T.contiguous(), dY[r]) + dhc
        o["dgates"][r], dcc = _gate_bwd32(dh, o["gates"][r], cc[t + 1], cc[t], dcc)
        o["daox"][r] = gemm("lstm.d", wx.T.contiguous(), o["dgates"][r])
        o["dhid"][r] = gemm("answer2.d", W["answer_processor.2.weight"].T.contiguous(), o["daox"][r, :256], mask=o["hid"][r])
        o["dans"][r] = gemm("answer0.d", a0w[:, :d["da"]].T.contiguous(), o["dhid"][r])
        o["dq2"][r] = gemm("query4.d", W["query.model.4.weight"].T.contiguous(), o["dq"][r], mask=o["q2"][r])
        o["dq1"][r] = gemm("query2.d", W["query.model.2.weight"].T.contiguous(), o["dq2"][r], mask=o["q1"][r])
        dhc = gemm("query0.d", W["query.model.0.weight"].T.contiguous(), o["dq1"][r]) + o["daox"][r, 256:]
    o["dcore_h0"], o["dcore_c0"] = dhc, dcc
    head_grads(hnext)
    gw = deinterleave(wg("lstm.w", o["dgates"], o["aox"]).T).T
    g["policy_core.weight_ih"], g["policy_core.weight_hh"] = gw[:, :256].contiguous(), gw[:, 256:].contiguous()
    g["policy_core.bias_ih"] = g["policy_core.bias_hh"] = deinterleave(o["dgates"]).sum(0)
    for name, layer, dA, X in (("answer_processor.2", "answer2.w", o["daox"][:, :256], o["hid"]),
                               ("answer_processor.0", "answer0.w", o["dhid"], ans),
                               ("query.model.4", "query4.w", o["dq"], o["q2"]), ("query.model.2", "query2.w", o["dq2"], o["q1"]),
                               ("query.model.0", "query0.w", o["dq1"], ch[:-1].reshape(F, 256))):
        g[name + ".weight"] = wg(layer, dA.contiguous(), X)[:, :P[name + ".weight"].shape[1]]
        g[name + ".bias"] = dA.sum(0)
    return o
