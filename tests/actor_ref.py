"""fp64 statement of the actor step chain (csrc/actor.hip: aaa_actor_step /
aaa_actor_step_core), stage by stage, with a per-element error bound for the
kernel that computes each stage, and a plain-float32 emulation of every stage
in the kernel's own partition with seeded single mistakes.

Every stage function takes the reference's own parameter tensors (the packed
layouts -- RGBx conv1 rows, the tap-major conv2 and ConvLSTM rows, the gate
interleave 4u + g -- are undone here, never read back) and the stage's input
AS THE CHAIN STORED IT (include/aaa.h AAA_ACT_WS_*, the step's outputs and
state), and returns (out64, bound): |kernel - out64| <= bound per element.
The shared pieces come from tests/tail_ref.py (lin, gates_of, gate_bound,
cell_from_gates, h_from, heads, the layer functions, U, TAU, Check),
tests/f32_split_ref.py (cnn_pieces, cnn_weights, cell_weights, recur_fwd, the
layout permutations), tests/attn_bf16_ref.py (readout64) and oracle/ref_cpu.py
(spatial_basis, grid_of, sample_actions).

Bounds.  u = 2^-24.  gamma(n) = eps + n u (1 + n u) with eps = u (a product is
rounded at most once), n the longest chain of fp32 additions a product passes
through, read off csrc/actor.hip:

  conv1 (k_act_vision)   "acc0 = mfma4(w1a[t], bv, acc0)" for t < 16: a wave
      chains 16 MFMAs of 4 products = 64 additions; "for (int k = 1; k < 4;
      ++k) s += red[k][tile][l]" = 3; "s[v] + p.b1[o0 + v]" = 1.   n1 = 68
  conv2 (k_act_vision)   "dot4(w2a[j], ya) + dot4(w2b[j], yb)" = 7 additions
      of 8 products; "for (int i = 0; i < 16; ++i) s += red2[wv][j][part * 16
      + i]" = 15 (the first adds to 0); two "__shfl_xor" = 2; "s + p.b2[o]" =
      1.                                                           n2 = 25
      y1 is never stored: the pair is checked as a composition,
      bound = gamma2 S2 + |W2| (gamma1 S1) + 2 u |X|, S2 on |y1| + gamma1 S1.
      Zero frame padding and a zero ring of conv1 outputs outside H1 x W1, as
      the reference's convolutions pad.
  ConvLSTM z (k_act_convlstm)   kLsSteps = 108 / 6 = 18 K blocks of 16 per
      slice, "acc0 = mfma4(a[v], b0[v], acc0)" for v < 4: 18 x 4 x 4 = 288
      chained products; "for (int k = 0; k < kActLstmKS; ++k) z[0] += ..." = 6;
      "z[e][0] + bias[0]" = 1.                                     n = 295
      gates: tail_ref.gate_bound (L (gamma S + 2 u |z|) + TAU); c and h from
      the STORED gates (io->gates): tail_ref.cell_from_gates / h_from.
  logits (k_act_attn)   "acc += kv[k][0] * Qq[4 * k] + ... + kv[k][3] * Qq[4
      * k + 3]" for k < 18: 72 additions.                           n = 72
  softmax (k_act_attn)   from the STORED logits, in fp64.  A weight is
      expf(l - m_c) expf(m_c - m) / t (the map: expf(l - m) / t), t = sum_c
      expf(m_c - m) s_c, s_c = sum_j expf(l_j - m_c).  Each exponent is an
      fp32 difference (u |l - m| relative in the exponential, |l - m| <=
      range = max l - min l), each expf within TAU_EXP relative; sums of
      non-negative terms keep the largest relative error of a term and add u
      per addition: s_c 6 (wsum), the product 1, t 2 + 6 (two chunks per lane,
      wsum), the division 1, the weight's product 1.  Relative error of a
      weight:  rho = 3 u range + 17 u + 3 TAU_EXP  (second order applied).
  readout (k_act_attn)   "acc += (j < np ? E[j][q] : 0.f) * vv[j]" for j < 16:
      the product and 15 additions; "acc += w * (partial)" over the chunks in
      groups of 8 (zero weights past nch): a product and nch8 - 1 additions.
      n = 16 + nch8;  bound = (rho + gamma(n)) sum_p alpha_p |V_p|.
      The query copy, prev_reward, prev_action and the zero padding are exact.
  one wave per output row (qlin_row, k_act_ans0, k_act_ans2, k_act_lstmcell,
      k_act_lstmcell_core, heads_draw): a lane's NIT float4 slices = 4 NIT
      products, "wsum" / the "__shfl_xor" butterfly = 6, the bias = 1:
      n = 4 NIT + 7 with NIT = 1 (query.0, query.2, LSTMCell zero state,
      heads), 2 (answer.2: w0, w1; the carried LSTMCell: wx, wh; query.4 at
      nq = 4: K = 288), 3 (query.4 at nq = 8: K = 576), 5 / 9 (answer.0 at
      nq = 4 / 8: "NIT = NQ == 4 ? 5 : 9").
      The LSTMCell stores neither its gates nor (zero state) its c: h is held
      to the gate bounds carried through c = f c' + i g~ and h = o tanh(c).
  carry   h (or h_out) is Hs bit for bit, core_h (or core_h_out) is LH, the
      ``query`` output is Q_t, and inputs are untouched when an _out is given.
  constant query (zero-state chain)   packed once by aaa_pack_weights, not by
      the chain: read back from the answer row's copy and held to the
      any-order bound n = K of the three layers on a zero input.

TAU_EXP: expf's error is not stated in a document this repository can cite,
so it was measured as tail_ref.TAU was: the worst relative error of the
attention map against the fp64 softmax of the stored logits on the MI355X
(tests/test_gpu_actor_pins.py test_expf_term_measured prints it; the map's
error holds three such terms and the exponents' roundings, so it overstates a
single expf), times 4, under tail_ref.TAU_CAP.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import attn_bf16_ref as AR
import f32_split_ref as SR
import tail_ref as R
from helpers import detinit
from oracle import ref_cpu
from tail_ref import TAU, TAU_CAP, U, Check, cdiv

# worst |map - softmax64(stored logits)| / softmax64 over test_expf_term_measured's cases on the MI355X
TAU_EXP_MEASURED = 2.362e-7
TAU_EXP = min(4 * TAU_EXP_MEASURED, TAU_CAP)
assert TAU_EXP <= TAU_CAP

CHUNK, MAX_CHUNKS, KS = 16, 128, 6   # actor.h kAttnChunk, kActMaxChunks, kActLstmKS
POISON = 1.0e4                       # finite: a stale row shows, a float4 load past a ragged edge stays finite
N1, N2, NZ, NL = 68, 25, 295, 72


def gamma(n):
    return U + n * U * (1 + n * U)


def wave_n(nit):
    return 4 * nit + 7


def nit_ans0(nq):
    return 5 if nq == 4 else 9


def nit_q4(nq):
    return cdiv(72 * nq, 256)


def n_table(nq, P):
    """Stage -> n (DESIGN.md "Actor chain: accuracy on its own operands")."""
    return {"conv1": N1, "conv2": N2, "convlstm.z": NZ, "logits": NL, "readout": 16 + cdiv(cdiv(P, CHUNK), 8) * 8,
            "query0": wave_n(1), "query2": wave_n(1), "query4": wave_n(nit_q4(nq)), "answer0": wave_n(nit_ans0(nq)),
            "answer2": wave_n(2), "lstm": wave_n(1), "lstm.carried": wave_n(2), "heads": wave_n(1)}


# --------------------------------------------------------------------- cases --
# (H, W, B, nq, A, core, u8, prev, oop): frame, rows, queries, actions, stateful core, uint8 frames,
# prev_reward / prev_action given, the checked second step out of place (h_out / c_out / core_*_out)
CASES = [
    (8, 8, 5, 4, 3, False, True, True, True),          # P = 1: softmax of one position; B = 5: wave 0 draws two rows
    (8, 8, 4, 8, 1, True, False, False, False),        # A = 1: draw_row's clamp
    (16, 16, 4, 8, 17, False, False, True, False),     # P = 4: under one chunk and one tile; 2A = 34: a 2-row last group
    (16, 16, 1, 4, 3, True, True, True, True),
    (64, 64, 5, 4, 18, True, True, False, True),       # P = 64: exact tile, exact chunks
    (64, 64, 1, 8, 17, False, False, True, False),
    (84, 84, 16, 4, 256, False, True, True, True),     # the workload's grid; lg[16 * 256] exactly full
    (84, 84, 16, 8, 256, True, False, True, False),
    (210, 160, 4, 4, 18, False, False, False, False),  # P = 540: non-square
    (210, 160, 1, 8, 18, True, True, True, True),
    (256, 256, 1, 4, 18, False, True, True, False),    # P = 1024: nch = 64
    (256, 256, 1, 8, 3, True, False, False, True),
    (264, 256, 1, 8, 18, False, False, True, True),    # P = 1056: nch = 66, the k = 1 half of mc[] / sc[] / Wc[]
    (264, 256, 1, 4, 17, True, True, True, False),
    (506, 256, 1, 8, 18, False, True, False, False),   # P = 2048: nch = 128 = kActMaxChunks
    (506, 256, 1, 4, 18, True, False, True, True),
]


def case_id(c):
    H, W, B, nq, A, core, u8, prev, oop = c
    return f"{H}x{W}_B{B}nq{nq}A{A}" + ("_core" if core else "") + ("_u8" if u8 else "_f32") + \
        ("" if prev else "_noprev") + ("_oop" if oop else "")


def geom(c):
    H, W, B, nq, A = c[:5]
    h, w = ref_cpu.grid_of(H, W)
    P = h * w
    ans_in = 256 * nq + 2
    return dict(H=H, W=W, B=B, nq=nq, A=A, h=h, w=w, P=P, nch=cdiv(P, CHUNK), npt=cdiv(P, 64), ans_in=ans_in,
                ans_ld=(ans_in + 7) // 8 * 8, qd=72 * nq)


assert [geom(c)["P"] for c in CASES[::2]] == [1, 4, 64, 121, 540, 1024, 1056, 2048]
assert {geom(c)["nch"] for c in CASES} >= {1, 4, 8, 34, 64, 66, MAX_CHUNKS}
assert {c[2] for c in CASES} == {1, 4, 5, 16} and {c[4] for c in CASES} == {1, 3, 17, 18, 256}
assert all(c[2] == 1 for c in CASES if geom(c)["P"] >= 1024)


@functools.lru_cache(maxsize=None)
def params(nq, A):
    """(name -> array as detinit gives it, name -> fp64 tensor)."""
    raw = detinit.deterministic_params(3, A, nq)
    return raw, {k: torch.from_numpy(np.asarray(v)).double() for k, v in raw.items()}


def rnd(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).float()


def inputs(c, step):
    """One step's host inputs: frames (B, H, W, 3) in the case's dtype, prev_reward / prev_action (or None)."""
    H, W, B, nq, A, core, u8, prev, _ = c
    fr = torch.from_numpy(detinit.frames_u8(900 + 7 * step + H, (B, H, W, 3)))
    if not u8:
        fr = fr.float() * SR.FRAME_SCALE
    pr = rnd(50 + step, (B,)) if prev else None
    pa = (torch.arange(B) * 7 + step).remainder(A).float() if prev else None
    return fr, pr, pa


def state0(c):
    """The non-zero carried state step 0 starts from: h, c (B, P, 128)[, core_h, core_c (B, 256)]."""
    g = geom(c)
    st = {"h": rnd(31, (g["B"], g["P"], 128), 0.5), "c": rnd(32, (g["B"], g["P"], 128), 1.0)}
    if c[5]:
        st["core_h"], st["core_c"] = rnd(33, (g["B"], 256), 0.5), rnd(34, (g["B"], 256), 1.0)
    return st


# -------------------------------------------------------------------- stages --
def _rows1024(x, per):
    """(M, per) pixel rows -> (ceil(M / 2), 2 per) and M: tail_ref's cell helpers take 256 units per row, the
    ConvLSTM has 128 channels per pixel, so two pixels make one row (an odd count is padded by a zero pixel)."""
    M = x.shape[0]
    if M % 2:
        x = torch.cat([x, torch.zeros(1, x.shape[1], dtype=x.dtype)])
    return x.reshape(-1, 2 * per), M


def vision(raw, frames):
    """frames (B, H, W, 3) -> X (B, P, 64): conv1 and conv2 as a composition (y1 is never stored)."""
    W64 = SR.cnn_weights(raw)
    w1, b1, w2, b2 = W64
    x = frames.double().permute(0, 3, 2, 1).contiguous()          # attention.py:179's transpose
    B = x.shape[0]
    h, w = ref_cpu.grid_of(frames.shape[1], frames.shape[2])
    r = SR.cnn_pieces(W64, x, torch.zeros(B, 64, w, h, dtype=torch.float64))
    S1 = F.conv2d(x.abs(), w1.abs(), b1.abs(), stride=4, padding=1)
    e1 = gamma(N1) * S1
    S2 = F.conv2d(r["y1"].abs() + e1, w2.abs(), b2.abs(), stride=2, padding=2)
    E = F.conv2d(e1, w2.abs(), None, stride=2, padding=2)
    bound = gamma(N2) * S2 + E + 2 * U * r["y2"].abs()
    return SR.from_ref(r["y2"]).reshape(B, -1, 64), SR.from_ref(bound).reshape(B, -1, 64)


def convlstm_pre(raw, X, h_in, hw):
    """Stored X (B, P, 64) and h_{t-1} (B, P, 128) -> the gate pre-activations (B*P, 512), row 4 ch + gate, and S."""
    h, w = hw
    B = X.shape[0]
    Wx, b, Wh = SR.cell_weights(raw)
    x = SR.to_ref(X.double().reshape(B * h * w, 64), B, h, w)
    hp = SR.to_ref(h_in.double().reshape(B * h * w, 128), B, h, w)
    z = F.conv2d(x, Wx, b, padding=1) + F.conv2d(hp, Wh, None, padding=1)
    S = F.conv2d(x.abs(), Wx.abs(), b.abs(), padding=1) + F.conv2d(hp.abs(), Wh.abs(), None, padding=1)
    return tuple(SR.gates_from_ref(t.reshape(B, 4, 128, w, h)) for t in (z, S))


def convlstm_gates(raw, X, h_in, hw):
    z, S = convlstm_pre(raw, X, h_in, hw)
    z2, M = _rows1024(z, 512)
    S2, _ = _rows1024(S, 512)
    g = R.gates_of(z2)[0].reshape(-1, 512)[:M]
    bound = R.gate_bound(z2, S2, gamma(NZ)).reshape(-1, 512)[:M]
    return g.reshape(X.shape[0], -1, 512), bound.reshape(X.shape[0], -1, 512)


def convlstm_c(gates, c_in):
    """c_t from the STORED gates (B, P, 512) and c_{t-1}."""
    g2, M = _rows1024(gates.reshape(-1, 512), 512)
    c2, _ = _rows1024(c_in.reshape(-1, 128), 128)
    c, b = R.cell_from_gates(g2, c2)
    return c.reshape(-1, 128)[:M].reshape(c_in.shape), b.reshape(-1, 128)[:M].reshape(c_in.shape)


def convlstm_h(gates, c):
    g2, M = _rows1024(gates.reshape(-1, 512), 512)
    c2, _ = _rows1024(c.reshape(-1, 128), 128)
    hh, b = R.h_from(g2, c2)
    return hh.reshape(-1, 128)[:M].reshape(c.shape), b.reshape(-1, 128)[:M].reshape(c.shape)


def attn_logits(Hs, S, Q):
    """Stored h_t (B, P, 128), the basis (P, 64) and the queries (B, nq, 72) -> logits (B, P, nq)."""
    K = torch.cat([Hs.double()[:, :, :8], S.double().expand(Hs.shape[0], -1, -1)], 2)
    Qd = Q.double()
    return K @ Qd.transpose(1, 2), gamma(NL) * (K.abs() @ Qd.abs().transpose(1, 2))


def softmax_rho(lg):
    """(the fp64 softmax over the positions of the STORED logits (B, P, nq), a weight's relative error (B, 1, nq))."""
    l = lg.double()
    rng = l.amax(1, keepdim=True) - l.amin(1, keepdim=True)
    rho = 3 * U * rng + 17 * U + 3 * TAU_EXP
    return torch.softmax(l, 1), rho * (1 + rho)


def attn_map(lg):
    """The map from the stored logits; 2^-126 absolute for a weight that leaves fp32's normal range."""
    A, rho = softmax_rho(lg)
    return A, A * rho + 2.0 ** -126


def answer_row(lg, Hs, S, Q, pr, pa, ans_ld):
    """The answer row (B, ans_ld) = [readout (nq x 184) | Q (nq x 72) | prev_reward | prev_action | 0] from the
    stored logits, h_t, basis and queries; the copies and the padding are exact (bound 0)."""
    B, P, nq = lg.shape
    A, rho = softmax_rho(lg)
    a = AR.readout64(A, Hs.double(), S.double())                                 # (B, nq * 184)
    Sa = AR.readout64(A, Hs.double().abs(), S.double().abs())
    n = 16 + cdiv(cdiv(P, CHUNK), 8) * 8
    ba = (rho.reshape(B, nq, 1) + gamma(n)).expand(B, nq, 184).reshape(B, -1) * Sa
    row = torch.zeros(B, ans_ld, dtype=torch.float64)
    bound = torch.zeros_like(row)
    row[:, :nq * 184], bound[:, :nq * 184] = a, ba
    row[:, nq * 184:nq * 256] = Q.double().reshape(B, -1)
    if pr is not None:
        row[:, nq * 256] = pr.double()
    if pa is not None:
        row[:, nq * 256 + 1] = pa.double()
    return row, bound


def _wave(o_S, nit):
    return o_S[0], R.gemm_bound(o_S[0], o_S[1], gamma(wave_n(nit)))


def query0(P, core_h): return _wave(R.query0(P, core_h), 1)
def query2(P, q1): return _wave(R.query2(P, q1), 1)
def query4(P, q2, nq): return _wave(R.query4(P, q2), nit_q4(nq))
def answer0(P, ans, nq): return _wave(R.answer0(P, ans), nit_ans0(nq))
def answer2(P, hid): return _wave(R.answer2(P, hid), 2)
def heads(P, lh): return _wave(R.heads(P, lh), 1)


def lstm_cell(P, ao, core=None):
    """AO (B, 256) [and the stored (core_h, core_c)] -> (go, e_go, c, e_c): the output gate, c = f c' + i g~ in
    fp64 and their bounds.  The kernel stores no gates: their bounds (tail_ref.gate_bound) are carried through
    the products, first and second order, plus 3 u for the two products and the addition."""
    x = ao if core is None else torch.cat([ao, core[0]], 1)
    z, S = R.lstm_pre(P, x, core is not None)
    g = R.gates_of(z)[0]
    eg = R.gate_bound(z, S, gamma(wave_n(1 if core is None else 2)))
    gi, gf, gc, go = g.reshape(-1, 256, 4).unbind(-1)
    ei, ef, ec, eo = eg.reshape(-1, 256, 4).unbind(-1)
    cp = core[1].double() if core is not None else torch.zeros_like(gi)
    a, b = gf * cp, gi * gc
    carried = cp.abs() * ef + gc.abs() * ei + gi.abs() * ec + ei * ec
    return go, eo, a + b, carried + 3 * U * (a.abs() + b.abs() + carried)


def lstm_h(go, eo, c, e_c):
    """h = o tanh(c) with |o' - o| <= eo, |c' - c| <= e_c (tanh is 1-Lipschitz), tanhf within TAU, the product 2 u."""
    t = torch.tanh(c)
    hh = go * t
    return hh, t.abs() * eo + (go.abs() + eo) * (e_c + TAU) + 2 * U * (hh.abs() + eo + e_c + TAU)


def const_query(P, nq):
    """QueryNetwork on the zero input (Q1), the constant query aaa_pack_weights stores: (Q (nq, 72), bound) for any
    summation order of each layer's K + 1 terms."""
    z = torch.zeros(1, 256, dtype=torch.float64)
    q1, _ = R.query0(P, z)                                     # relu(bias): exact
    q2, S2 = R.query2(P, q1)
    e2 = R.gemm_bound(q2, S2, gamma(129))
    q, S4 = R.query4(P, q2)
    W4 = P["query.model.4.weight"].double().abs()
    e4 = gamma(72 * nq + 1) * (S4 + e2 @ W4.T) + e2 @ W4.T + 2 * U * q.abs()
    return q.reshape(nq, 72), e4.reshape(nq, 72)


# -------------------------------------------------------------------- checks --
def check(o, c, what=""):
    """Every stage of one step ``o`` (the GPU test fills it from the workspace regions, the outputs and the state
    of a run; ``emulate`` from float32 arithmetic on the CPU) against fp64 on the operands it stored."""
    H, W, B, nq, A, core, u8, prev, oop = c
    g = geom(c)
    raw, P = params(nq, A)
    ck = Check(f"{case_id(c)} {what}".strip())
    ck("vision", o["X"], *vision(raw, o["frames"].float()))
    ck("convlstm.gates", o["gates"], *convlstm_gates(raw, o["X"], o["h_in"], (g["h"], g["w"])))
    ck("convlstm.c", o["c"], *convlstm_c(o["gates"], o["c_in"]))
    ck("convlstm.h", o["Hs"], *convlstm_h(o["gates"], o["c"]))
    ck.exact("h carry", o["h_carry"], o["Hs"])
    S = o["S"]
    Q = o["ans"][:, nq * 184:nq * 256].reshape(B, nq, 72)       # the row's copy of the queries the readout used
    if core:
        ck("query0", o["q1"], *query0(P, o["core_h_in"]))
        ck("query2", o["q2"], *query2(P, o["q1"]))
        ck("query4", o["qt"], *query4(P, o["q2"], nq))
        ck.exact("answer row Q copy", Q, o["qt"])
        if o.get("query_out") is not None:
            ck.exact("query output", o["query_out"], o["qt"])
    else:
        qc, bq = const_query(P, nq)
        ck("const query", Q, qc.expand(B, nq, 72), bq.expand(B, nq, 72))
    ck("logits", o["lg"], *attn_logits(o["Hs"], S, Q))
    if o.get("attn") is not None:
        ck("map", o["attn"], *attn_map(o["lg"]))
    ck("answer row", o["ans"], *answer_row(o["lg"], o["Hs"], S, Q, o["pr"], o["pa"], g["ans_ld"]))
    ck("answer0", o["hid1"], *answer0(P, o["ans"], nq))
    ck("answer2", o["AO"], *answer2(P, o["hid1"]))
    if core:
        go, eo, cl, e_c = lstm_cell(P, o["AO"], (o["core_h_in"], o["core_c_in"]))
        ck("lstm.c", o["core_c_out"], cl, e_c)
        ck("lstm.h", o["LH"], *lstm_h(go, eo, o["core_c_out"].double(), torch.zeros_like(go)))   # from the stored c
        ck.exact("core_h carry", o["core_h_out"], o["LH"])
    else:
        ck("lstm.h", o["LH"], *lstm_h(*lstm_cell(P, o["AO"])))
    ck("heads", torch.cat([o["logits"], o["values"]], 1), *heads(P, o["LH"]))
    return ck


# ----------------------------------------------- emulation (CPU, float32) -----
FAULTS = ("conv1_pad_clamped", "conv2_ring_bias", "convlstm_slice_dropped", "convlstm_pad_pixel0",
          "readout_clamped_rows_weighted", "merge_first_64_chunks", "merge_own_max", "prev_swapped",
          "clamped_slice_twice", "heads_pad_row_wraps", "lstm_gate_major", "lstm_fc_dropped", "h_copy_last_share")


def _butterfly(acc):
    """wsum: v += shfl_xor(v, o) for o = 32 .. 1 over the last (lane) axis; every lane ends with the sum."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    return acc[..., 0]


def _wave_rows(Wt, x, nit, bias, twice=False):
    """One wave per output row: NIT float4 slices per lane at offsets min(4 lane + 256 i, K - 4), a slice counted
    where 4 lane + 256 i < K (``twice``: the guard lost, the clamped last slice counted again), the butterfly, the
    bias.  Wt (N, K), x (B, K) float32 -> (B, N)."""
    K = Wt.shape[1]
    lane = torch.arange(64)
    acc = torch.zeros(x.shape[0], Wt.shape[0], 64)
    for i in range(nit):
        k0 = 4 * lane + 256 * i
        idx = torch.minimum(k0, torch.tensor(K - 4))[:, None] + torch.arange(4)
        d = torch.einsum("nlj,blj->bnl", Wt[:, idx], x[:, idx])
        on = torch.ones(64, dtype=torch.bool) if twice else k0 < K
        acc = acc + torch.where(on, d, torch.zeros_like(d))
    return _butterfly(acc) + bias


def _emu_vision(raw, frames, fault):
    """k_act_vision in the kernel's own orientation (rows = frame rows): conv1 as four K quarters of 16 taps
    summed in order, conv2 with lanes along K (8 products each), 16-term parts and two shuffles."""
    w1, b1, w2, b2 = (t.float() for t in SR.cnn_weights(raw, torch.float32))
    w1, w2 = w1.transpose(2, 3), w2.transpose(2, 3)                 # (o, c, ky, kx) on (H, W) images
    x = frames.float().permute(0, 3, 1, 2)                          # (B, 3, H, W)
    B = x.shape[0]
    xp = F.pad(x, (1, 1, 1, 1), mode="replicate" if fault == "conv1_pad_clamped" else "constant")
    H1, W1 = (xp.shape[2] - 8) // 4 + 1, (xp.shape[3] - 8) // 4 + 1
    cols = F.unfold(xp, 8, stride=4).reshape(B, 3, 64, H1 * W1)     # (c, tap = ky * 8 + kx)
    wt = w1.reshape(32, 3, 64)
    y1 = torch.zeros(B, 32, H1 * W1)
    for q in range(4):
        t = slice(16 * q, 16 * q + 16)
        y1 = y1 + torch.einsum("oct,bctp->bop", wt[:, :, t], cols[:, :, t])
    y1 = (y1 + b1[None, :, None]).reshape(B, 32, H1, W1)
    ring = F.pad(y1, (2, 2, 2, 2))
    if fault == "conv2_ring_bias":
        inside = F.pad(torch.ones(1, 1, H1, W1), (2, 2, 2, 2)) > 0
        ring = torch.where(inside, ring, b1[None, :, None, None].expand_as(ring))
    h, w = (H1 + 4 - 4) // 2 + 1, (W1 + 4 - 4) // 2 + 1
    c2 = F.unfold(ring, 4, stride=2).reshape(B, 32, 16, h * w).transpose(1, 2).reshape(B, 64, 8, h * w)   # K = tap * 32 + ci
    wk = w2.reshape(64, 32, 16).transpose(1, 2).reshape(64, 64, 8)
    lanes = torch.einsum("olk,blkp->bopl", wk, c2)                  # (B, o, P, lane)
    parts = torch.zeros(B, 64, h * w, 4)
    for i in range(16):
        parts = parts + lanes.reshape(B, 64, h * w, 4, 16)[..., i]
    s = (parts[..., 0] + parts[..., 1]) + (parts[..., 2] + parts[..., 3])
    return (s + b2[None, :, None]).transpose(1, 2).contiguous()     # (B, P, 64)


def _emu_convlstm(raw, X, h_in, c_in, hw, fault):
    """k_act_convlstm: K = tap * 192 + [x | h] channel, six slices of 288 summed in slice order, then the cell."""
    h, w = hw
    B, P = X.shape[0], h * w
    Wx, b, Wh = (t.float() for t in SR.cell_weights(raw, torch.float32))
    Wk = torch.cat([Wx, Wh], 1).transpose(2, 3).permute(0, 2, 3, 1).reshape(512, 1728)   # gate-major rows
    xh = torch.cat([X, h_in], 2).reshape(B, h, w, 192).permute(0, 3, 1, 2)
    cols = F.unfold(F.pad(xh, (1, 1, 1, 1)), 3).reshape(B, 192, 9, P)
    if fault == "convlstm_pad_pixel0":   # a padding tap keeps the clamped load of pixel 0
        inside = F.unfold(F.pad(torch.ones(1, 1, h, w), (1, 1, 1, 1)), 3).reshape(1, 1, 9, P) > 0
        cols = torch.where(inside, cols, xh[:, :, 0, 0][:, :, None, None].expand_as(cols))
    cols = cols.transpose(1, 2).reshape(B, 1728, P)
    z = torch.zeros(B, 512, P)
    for ks in range(KS):
        if fault == "convlstm_slice_dropped" and ks == KS - 1:
            continue
        k = slice(288 * ks, 288 * ks + 288)
        z = z + Wk[:, k] @ cols[:, k]
    z = (z + b[None, :, None]).reshape(B, 4, 128, P)
    gi, gf, go = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.sigmoid(z[:, 3])
    gc = torch.tanh(z[:, 2])
    cp = c_in.transpose(1, 2)
    c = gf * cp + gi * gc
    hh = go * torch.tanh(c)
    gates = torch.stack([gi, gf, gc, go], -1).permute(0, 2, 1, 3).reshape(B, P, 512)     # row 4 ch + gate
    return gates.contiguous(), c.transpose(1, 2).contiguous(), hh.transpose(1, 2).contiguous()


def _emu_attn(Hs, S, Q, pr, pa, ans_ld, fault):
    """k_act_attn: logits, per-chunk max / sum / partial readout, the merge in chunk order, the answer row, the map."""
    B, P, nq = Hs.shape[0], Hs.shape[1], Q.shape[1]
    nch = cdiv(P, CHUNK)
    K = torch.cat([Hs[:, :, :8], S.expand(B, -1, -1)], 2)
    V = torch.cat([Hs[:, :, 8:], S.expand(B, -1, -1)], 2)
    lg = K @ Q.transpose(1, 2)
    pad = nch * CHUNK - P
    lp = F.pad(lg, (0, 0, 0, pad), value=float("-inf")).reshape(B, nch, CHUNK, nq)
    Vp = F.pad(V, (0, 0, 0, pad)).reshape(B, nch, CHUNK, 184)
    mc = lp.amax(2)
    e = torch.exp(lp - mc[:, :, None])
    sc = torch.zeros(B, nch, nq)
    for j in range(CHUNK):
        sc = sc + e[:, :, j]
    if fault == "readout_clamped_rows_weighted" and pad:   # rows past np are copies of row np - 1: given its weight
        npl = CHUNK - pad
        e = e.clone()
        e[:, -1, npl:] = e[:, -1, npl - 1:npl]
        Vp = Vp.clone()
        Vp[:, -1, npl:] = Vp[:, -1, npl - 1:npl]
    part = torch.zeros(B, nch, nq, 184)
    for j in range(CHUNK):
        part = part + e[:, :, j, :, None] * Vp[:, :, j, None, :]
    live = nch if fault != "merge_first_64_chunks" else min(nch, 64)
    m = mc[:, :live].amax(1)
    wexp = torch.exp(mc - m[:, None]) if fault != "merge_own_max" else torch.ones_like(mc)
    wexp[:, live:] = 0
    t = torch.zeros(B, nq)
    for cc in range(nch):
        t = t + wexp[:, cc] * sc[:, cc]
    inv = 1.0 / t
    Wc = wexp * inv[:, None]
    acc = torch.zeros(B, nq, 184)
    for cc in range(nch):
        acc = acc + Wc[:, cc, :, None] * part[:, cc]
    row = torch.zeros(B, ans_ld)
    row[:, :nq * 184] = acc.reshape(B, -1)
    row[:, nq * 184:nq * 256] = Q.reshape(B, -1)
    r = pr if pr is not None else torch.zeros(B)
    a = pa if pa is not None else torch.zeros(B)
    if fault == "prev_swapped":
        r, a = a, r
    row[:, nq * 256], row[:, nq * 256 + 1] = r, a
    amap = torch.exp(lg - m[:, None]) * inv[:, None]
    return lg.contiguous(), amap, row


def emulate(c, fault=None, step=0, state=None):
    """One step of the chain in plain float32 on the CPU, each stage in its kernel's partition (K quarters and
    slices, position chunks with the max / sum merge, clamped float4 slices, 8-row head groups), on ``inputs(c,
    step)`` from ``state`` (default ``state0(c)``).  ``fault``: one of FAULTS seeded into the stage it belongs to.
    Returns the run dict ``check`` takes."""
    assert fault is None or fault in FAULTS
    H, W, B, nq, A, core, u8, prev, oop = c
    g = geom(c)
    raw, P = params(nq, A)
    Wf = {k: v.float() for k, v in P.items()}
    st = state if state is not None else state0(c)
    fr, pr, pa = inputs(c, step)
    S = ref_cpu.spatial_basis(g["h"], g["w"]).reshape(g["P"], 64)
    o = {"frames": fr, "pr": pr, "pa": pa, "S": S, "h_in": st["h"], "c_in": st["c"]}
    o["X"] = _emu_vision(raw, fr, fault)
    o["gates"], o["c"], o["Hs"] = _emu_convlstm(raw, o["X"], st["h"], st["c"], (g["h"], g["w"]), fault)
    o["h_carry"] = o["Hs"].clone()
    if fault == "h_copy_last_share":   # k_act_attn: chunk c copies float4s [c per, (c + 1) per) of the frame's P * 32
        per = cdiv(g["P"] * 32, g["nch"])
        o["h_carry"].reshape(B, -1)[:, 4 * (g["nch"] - 1) * per:] = st["h"].reshape(B, -1)[:, 4 * (g["nch"] - 1) * per:]
    twice = fault == "clamped_slice_twice"
    if core:
        o["core_h_in"], o["core_c_in"] = st["core_h"], st["core_c"]
        o["q1"] = _wave_rows(Wf["query.model.0.weight"], st["core_h"], 1, Wf["query.model.0.bias"], twice).clamp_min(0)
        o["q2"] = _wave_rows(Wf["query.model.2.weight"], o["q1"], 1, Wf["query.model.2.bias"], twice).clamp_min(0)
        o["qt"] = _wave_rows(Wf["query.model.4.weight"], o["q2"], nit_q4(nq), Wf["query.model.4.bias"], twice)
        o["query_out"] = o["qt"].clone()
        Q = o["qt"].reshape(B, nq, 72)
    else:
        Q = const_query(P, nq)[0].float().expand(B, nq, 72)
    o["lg"], o["attn"], o["ans"] = _emu_attn(o["Hs"], S, Q, pr, pa, g["ans_ld"], fault)
    a0w = torch.zeros(512, g["ans_ld"])
    a0w[:, :g["ans_in"]] = Wf["answer_processor.0.weight"]
    o["hid1"] = _wave_rows(a0w, o["ans"], nit_ans0(nq), Wf["answer_processor.0.bias"], twice).clamp_min(0)
    w2 = Wf["answer_processor.2.weight"]
    o["AO"] = _butterfly((w2.reshape(256, 64, 8)[None] * o["hid1"].reshape(B, 1, 64, 8)).sum(-1)) + Wf["answer_processor.2.bias"]
    wl = Wf["policy_core.weight_ih"]
    x = o["AO"]
    if core:
        wl, x = torch.cat([wl, Wf["policy_core.weight_hh"]], 1), torch.cat([o["AO"], st["core_h"]], 1)
    zl = _wave_rows(wl, x, 2 if core else 1, Wf["policy_core.bias_ih"] + Wf["policy_core.bias_hh"])   # gate-major
    z4 = (zl if fault == "lstm_gate_major" else R.interleave(zl)).reshape(B, 256, 4)
    gi, gf, go = torch.sigmoid(z4[..., 0]), torch.sigmoid(z4[..., 1]), torch.sigmoid(z4[..., 3])
    gc = torch.tanh(z4[..., 2])
    cprev = st["core_c"] if core else torch.zeros(B, 256)
    cl = gi * gc if fault == "lstm_fc_dropped" else gf * cprev + gi * gc
    o["LH"] = go * torch.tanh(cl)
    if core:
        o["core_c_out"], o["core_h_out"] = cl, o["LH"].clone()
    whd = torch.cat([Wf["policy_head.0.weight"], Wf["values_head.0.weight"]])
    bhd = torch.cat([Wf["policy_head.0.bias"], Wf["values_head.0.bias"]])
    lv = _wave_rows(whd, o["LH"], 1, bhd)
    if fault == "heads_pad_row_wraps" and (2 * A) % 8:   # a row past 2A (packed zero padding) stored through the clamped index
        lv = lv.clone()
        lv[:, 2 * A - 1] = 0.0
    o["logits"], o["values"] = lv[:, :A].contiguous(), lv[:, A:].contiguous()
    return o


def next_state(c, o):
    st = {"h": o["h_carry"], "c": o["c"]}
    if c[5]:
        st["core_h"], st["core_c"] = o["core_h_out"], o["core_c_out"]
    return st
