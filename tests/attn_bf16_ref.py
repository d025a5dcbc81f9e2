"""Inputs, fp64 references and the two-part emulation shared by the bf16
attention-readout tests (test_attn_bf16_emulation.py on the CPU,
test_gpu_attn_bf16.py on the GPU).

The bf16 learner's readout multiplies fp32 operands on a bf16 MFMA by cutting
each into hi + mid + lo bf16 parts and summing every part product in fp32
(csrc/attn_mfma.h): the result is that of fp32 FMAs up to summation order.  A
kernel that lost a low part would still pass the project's 1e-4 gate (both low
parts gone: about 1.5e-3 against the 2e-2 whole-model gate; the lo part gone:
a few 1e-6).  ``e2`` is the error such a kernel would make on a case's own
inputs -- the same quantity with the fp32 operands cut to TWO parts (hi =
bf16(x), mid = bf16(x - hi)), every part product summed in fp64 -- and the
tests hold a kernel to e2 / 2 and plain fp32 CPU arithmetic to e2 / 4.

Quantities (one frame: P positions, V = [O[:, 8:] | S] (P,184), K = [O[:, :8] | S] (P,72)):
  forward   readout[q] = sum_p A[p][q] V[p]                  operands cut: A, S
            its basis columns readout[q][120:]                operand cut: S (fwdS_e2)
  backward  dA = V da^T                                       operands cut: S, da
            dlogit = A (dA - sum_p A dA)
            dO_key = dlogit Q[:, :8],  dQ = dlogit^T K        (fp32 FMAs in every kernel: not cut)
            dO_key from a gradient on the basis columns only  operand cut: S (bwdS_e2)
"""
from __future__ import annotations

import functools

import torch

from helpers import rel_err
from oracle import ref_cpu

F = 3
# (h, w) given straight to the entry; P = h*w
GRIDS = [(3, 5),     # 15: under one 16-position block and one 32-position chunk (the LDS image at its 32-row floor)
         (8, 8),     # 64: P equals the padded length and the chunk count the stage depth -- no padding at all
         (11, 11),   # 121: configs 3 and 4
         (16, 16),   # 256: last P on the "<= 256" side of the backward dispatch
         (17, 16),   # 272: first past it; a partly filled second logits slot
         (16, 32),   # 512: both logits slots full, the "> 512" loop empty
         (19, 27),   # 513: exactly one position in the "> 512" loop
         (21, 21),   # 441: config 5
         (27, 20)]   # 540: the reference's default 210x160 frame
BASIS_ONLY_GRIDS = GRIDS[1:]   # the backward's basis-only case: 3x5's basis is mostly short binary fractions
NQS = [4, 8]
O_LD, O_OFF = 192, 64     # the learner's [x | h] rows: pitch 192, h at element 64
POISON = 1e4              # finite: the VALU kernels' 16-B loads may touch 8 elements past the h half


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def split2(x: torch.Tensor) -> torch.Tensor:
    """fp32 x cut to its first two bf16 parts, as fp64."""
    hi = x.to(torch.bfloat16).float()
    mid = (x - hi).to(torch.bfloat16).float()
    return hi.double() + mid.double()


def readout64(A, O, S):
    """(F,P,nq), (F,P,128), (P,64) fp64 -> (F, nq*184)."""
    V = torch.cat([O[:, :, 8:], S.expand(O.shape[0], -1, -1)], dim=2)
    return torch.matmul(A.transpose(1, 2), V).reshape(O.shape[0], -1)


def s_cols(readout, nq: int):
    """The basis columns (120..183 of each query's 184) of a (F, nq*184) readout."""
    return readout.reshape(readout.shape[0], nq, 184)[:, :, 120:]


def backward64(A, O, S, Q, da, S_dA=None, da_dA=None):
    """The explicit backward formulas in the dtype of the inputs: (dO_key (F,P,8), dQ (F,nq,72))
    without the answer row's copy of Q.  S_dA / da_dA: the operands of the dA product, if cut."""
    Fr = O.shape[0]
    Sf = S.expand(Fr, -1, -1)
    V = torch.cat([O[:, :, 8:], (S if S_dA is None else S_dA).expand(Fr, -1, -1)], dim=2)
    dA = torch.matmul(V, (da if da_dA is None else da_dA).transpose(1, 2))          # (F,P,nq)
    dlogit = A * (dA - (A * dA).sum(dim=1, keepdim=True))
    dO_key = torch.matmul(dlogit, Q[:, :, :8])
    dQ = torch.matmul(dlogit.transpose(1, 2), torch.cat([O[:, :, :8], Sf], dim=2))
    return dO_key, dQ


@functools.lru_cache(maxsize=None)
def case(hw, nq: int, per_frame_q: bool):
    """Inputs and references of one (grid, nq, query mode); read-only, shared by every test."""
    h, w = hw
    P = h * w
    c = {"h": h, "w": w, "P": P, "nq": nq, "per_frame_q": per_frame_q}
    c["O"] = rnd((F, P, 128), 1, 2.0).to(torch.bfloat16)
    c["S"] = ref_cpu.spatial_basis(h, w).reshape(P, 64).contiguous()
    c["Q"] = rnd((F if per_frame_q else 1, nq, 72), 2, 0.5).expand(F, nq, 72).contiguous()
    c["pr"], c["pa"] = rnd((F,), 3), torch.arange(F, dtype=torch.float32) % 18
    c["dans"] = rnd((F, 256 * nq + 2), 4)
    O64, S64, Q64 = c["O"].double(), c["S"].double(), c["Q"].double()
    c["O64"], c["S64"], c["Q64"] = O64, S64, Q64
    # fp64 oracle of the forward and, for both add_q, of the backward
    Or, Qr = O64.reshape(F, h, w, 128).clone().requires_grad_(True), Q64.clone().requires_grad_(True)
    A, answer = ref_cpu.attention_readout(Or, S64.reshape(h, w, 64), Qr, c["pr"], c["pa"])
    c["A64"], c["answer64"] = A.detach().reshape(F, P, nq), answer.detach()
    for add_q, ncol in ((0, nq * 184), (1, nq * 256)):
        gO, gQ = torch.autograd.grad((answer[:, :ncol] * c["dans"][:, :ncol].double()).sum(), (Or, Qr),
                                     retain_graph=True)
        c["dO64", add_q], c["dQ64", add_q] = gO.reshape(F, P, 128), gQ
    # the backward's map input: the oracle's, rounded to fp32 (independent of the forward kernel)
    c["A32"] = c["A64"].float()
    A32d, da = c["A32"].double(), c["dans"][:, :nq * 184].reshape(F, nq, 184)
    c["da"] = da
    # forward readout of that map: exact, two-part, plain fp32
    ro = readout64(A32d, O64, S64)
    c["fwd_e2"] = rel_err(readout64(split2(c["A32"]), O64, split2(c["S"])), ro)
    ro32 = readout64(c["A32"], c["O"].float(), c["S"])
    c["fwd_f32"] = rel_err(ro32, ro)
    # ... and its basis columns alone with only S cut: in fwd_e2 the map's cut dominates (it reaches all 184
    # columns), so a lost low part of S, which reaches these 64, stays below fwd_e2 / 2 and needs its own bound
    c["fwdS_e2"] = rel_err(s_cols(readout64(A32d, O64, split2(c["S"])), nq), s_cols(ro, nq))
    c["fwdS_f32"] = rel_err(s_cols(ro32, nq), s_cols(ro, nq))
    # backward from that map
    ex = backward64(A32d, O64, S64, Q64, da.double())
    two = backward64(A32d, O64, S64, Q64, da.double(), split2(c["S"]), split2(da))
    f32 = backward64(c["A32"], c["O"].float(), c["S"], c["Q"], da)
    c["bwd64"] = ex
    c["bwd_e2"] = tuple(rel_err(t, e) for t, e in zip(two, ex))
    c["bwd_f32"] = tuple(rel_err(t, e) for t, e in zip(f32, ex))
    # ... and from an answer gradient that reaches the basis columns only (dA = S da_S^T), S cut alone: in
    # bwd_e2 the cut of da dominates (it reaches all 184 columns of the sum), so a lost low part of S stays
    # below bwd_e2 / 2 (0.35 of it at worst) and needs its own case and bound
    c["dansS"] = c["dans"].clone()
    for q in range(nq):
        c["dansS"][:, q * 184:q * 184 + 120] = 0
    daS = c["dansS"][:, :nq * 184].reshape(F, nq, 184)
    gO, gQ = torch.autograd.grad((answer[:, :nq * 184] * c["dansS"][:, :nq * 184].double()).sum(), (Or, Qr))
    c["dO64", "S"], c["dQ64", "S"] = gO.reshape(F, P, 128), gQ
    exS = backward64(A32d, O64, S64, Q64, daS.double())
    twoS = backward64(A32d, O64, S64, Q64, daS.double(), split2(c["S"]), None)
    f32S = backward64(c["A32"], c["O"].float(), c["S"], c["Q"], daS)
    c["bwdS64"] = exS
    c["bwdS_e2"] = tuple(rel_err(t, e) for t, e in zip(twoS, exS))
    c["bwdS_f32"] = tuple(rel_err(t, e) for t, e in zip(f32S, exS))
    return c
