"""The bf16 ConvLSTM recurrence kernels held to fp64 on their own stored operands,
step by step (tests/convlstm_bf16_ref.py: the references, the bounds (a)-(d) and
their derivations; tests/test_convlstm_bf16_emulation.py: the CPU evidence):

  * the frame-resident forward and BPTT (one workgroup per frame:
    k_convlstm_fwd_frames G = 1, k_convlstm_bwd_frames<0, false>),
  * the paired ones (two per frame: G = 2, k_convlstm_bwd_pairs),
  * band mode on the 21x21 grid (k_convlstm_fwd_frames BAND,
    k_convlstm_bwd_frames<0, true>),
  * the per-step launches (EpiConvLstmFwd / EpiConvLstmBwd with the batched dx),
    behind a per-step and behind a frame-resident forward, and on the 21x21 grid,
  * the bf16 weight gradient (register-staged, and the LDS-DMA ring where the
    pixel rows are whole K tiles), also at the K-loop edges of 75, 363, 540 rows,
  * the cell component entry (aaa_convlstm_cell_fwd / _bwd, bf16).

Every learner test runs ONE forward and ONE phased backward (HEAD, then CORE with
dhT / dcT where the case carries state) of at most 20 frames, reads every stored
buffer back through the AAA_BF16_WS_* regions, de-permutes the channel-quad-major
slices by aaa_core_layout's mask, asserts from the timer variants that the kernel
it names is the one that ran, and ends on a clean pair status.  Each observable's
err / gate (and mismatch share) is printed before it is asserted.

Reference: attention.py:110-126 (ConvLSTMCell.forward) over T steps and its
autograd backward (main_mp.py:77).  Measured ratios: DESIGN.md "bf16 ConvLSTM:
accuracy on its own operands".
"""
import ctypes

import pytest
import torch

import convlstm_bf16_ref as C
import f32_split_ref as R
import vision_bf16_ref as V
from helpers import detinit
from oracle import ref_cpu
from test_gpu_parity import _agent, _cot

import attention
from aaa_amd.runtime import CellRunner

pytestmark = pytest.mark.gpu
N = attention._pkg._native
PARAMS = detinit.deterministic_params(0, 18)

# selection -> (AAA_FRAMES_FWD, AAA_FRAMES_BWD)
SELECT = {"frames": ("1", "1"), "pairs": ("2", "2"), "frames-fwd+steps": ("1", "0"), "steps": ("0", "0")}


def _learner(cuda, monkeypatch, case, env):
    """One forward and phased backward of a bf16 UnrollRunner under ``env``; every stored buffer read back through
    the new regions, row-major on the host (the dict convlstm_bf16_ref.check reads)."""
    T, B, H, W, state = case
    for k in ("AAA_FRAMES_FWD", "AAA_FRAMES_BWD", "AAA_FRAMES_BAND"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, w = ref_cpu.grid_of(H, W)
    P, M = h * w, B * h * w
    assert T * B <= 20
    ag = _agent(cuda, grid=(h, w), conv_dtype="bf16")
    r = ag._runner(B, T, H, W, cuda, False, False)
    S = ag._basis_for(r.h, r.w, H, W, cuda)
    flat, packed = ag._packed_params(r, list(ag.parameters()))
    X = R.frames(T, B, H, W, C.FRAME_SCALE).to(cuda)
    h0 = c0 = dhT = dcT = None
    if state:
        h0, c0 = R.state_in(B, h, w)
    gdt, mask = r.core_layout()
    ws = r.new_workspace()
    o = {"T": T, "B": B, "h": h, "w": w, "mask": mask, "dhT": None, "dcT": None}
    reg = lambda region, shape, dt: r.workspace_region(ws, region, shape, dt).cpu()   # noqa: E731
    N.pair_status(clear=True)
    N.timing_enable(True)
    try:
        _, _, _, hT, cT = r.forward(flat, packed, S, X, ws, h0=None if h0 is None else h0.to(cuda),
                                    c0=None if c0 is None else c0.to(cuda), want_attn=False, want_state=True)
        o["fvar"] = N.timing_stats(N.TIMER_FWD_STEP)["variant"]
        o["xh"] = reg(N.BF16_WS_XH, (T + 1, M, 192), torch.bfloat16)
        c = reg(N.BF16_WS_C, (T + 1, M, 128), torch.float32)
        gates = reg(N.BF16_WS_GATES, (T, M, 512), gdt)
        o["c"] = C.from_cqm4(c, P) if mask & N.CQM_C else c
        o["gates"] = C.from_cqmg(gates, P) if mask & N.CQM_G else gates
        o["hT"], o["cT"] = hT.cpu().reshape(M, 128), cT.cpu().reshape(M, 128)
        if mask == 0:   # row-major: aaa_core_export hands out the same bytes
            exp = [torch.empty(s, device=cuda, dtype=d) for s, d in zip(r.core_shapes(T), r.core_dtypes())]
            r.core_export(ws, 0, T, *exp)
            assert torch.equal(exp[0].cpu(), o["gates"]) and torch.equal(exp[1].cpu(), o["c"][1:])
            assert torch.equal(exp[2].cpu(), o["xh"][1:, :, 64:])
        else:
            assert r.core_dtypes() is None
        Gl, Gv = (g.to(cuda) for g in _cot(T, B))
        g, _, _ = r.backward(flat, packed, S, X, ws, Gl, Gv, phases=N.BWD_HEAD)
        dO = reg(N.BF16_WS_DO, (T, M, 128), torch.float32)
        o["dO"] = C.from_cqm4(dO, P) if mask & N.CQM_DO else dO
        if state:   # at the scale of the readout's cotangent
            dhT, dcT = (t.reshape(M, 128) for t in R.state_cot(B, h, w, float(o["dO"].abs().max())))
            o["dhT"], o["dcT"] = dhT, dcT
        g, dh0, dc0 = r.backward(flat, packed, S, X, ws, Gl, Gv, dhT=None if dhT is None else dhT.to(cuda),
                                 dcT=None if dcT is None else dcT.to(cuda), grads=g, want_state_grads=True,
                                 phases=N.BWD_CORE)
        o["bvar"] = N.timing_stats(N.TIMER_BPTT_STEP)["variant"]
        o["wvar"] = N.timing_stats(N.TIMER_CORE_WGRAD)["variant"]
        o["xvar"] = N.timing_stats(N.TIMER_CORE_DX)["variant"]
        o["dz"] = reg(N.BF16_WS_DZ, (T, M, 512), torch.bfloat16)
        o["dx"] = reg(N.BF16_WS_DX, (T, M, 64), torch.bfloat16)
        o["dh0"], o["dc0"] = dh0.cpu().reshape(M, 128), dc0.cpu().reshape(M, 128)
        lstm = g[r.offsets[4]:r.offsets[16]]   # the 12 ConvLSTM tensors, state_dict order
        assert lstm.numel() == 4 * (128 * 64 * 9 + 128 + 128 * 128 * 9) and r.sizes[3] == 64
        o["grads"] = R.split_cell_grads(lstm)
        o["gb2"] = g[r.offsets[3]:r.offsets[3] + 64].cpu()   # vision_cnn.1.bias: the column sum of dx
    finally:
        N.timing_enable(False)
    resident = "frame-resident BPTT" in o["bvar"]
    # which c_t the gate backward reads, and where the gate bias is summed (convlstm_bf16_ref's docstring): every
    # per-step BPTT tile that serves fp16 gates is a ring tile (csrc/step_tiles.h BpttTiles, kG16: all RingOnly)
    o["ccur"] = "recomputed" if resident else "stored"
    o["gb_sum"] = "fp32" if resident or gdt == torch.float16 else "either"
    if state:   # the state the kernels started from: h0 rounded to bf16 in slot 0, c0 as given
        assert torch.equal(o["xh"][0, :, 64:], h0.reshape(M, 128).to(torch.bfloat16))
        assert torch.equal(o["c"][0], c0.reshape(M, 128))
    else:
        assert not o["xh"][0, :, 64:].any() and not o["c"][0].any()
    # the state handed back is the last stored step: h_{T-1} as the bf16 the next step would read, c_{T-1}
    assert torch.equal(o["hT"], o["xh"][T, :, 64:].float()) and torch.equal(o["cT"], o["c"][T])
    return o


def _steps(var):
    return var.startswith("bf16") and "step" in var and "EpiConvLstmFwd" in var and "frame-resident" not in var


def _check(o, what, wgrad_only=False):
    rep, bad = C.check(o, C.CAP_DEV, what=what, wgrad_only=wgrad_only)
    assert not bad, bad
    assert N.pair_status(clear=True) == 0
    return rep


def _wgrad_variant_ok(o):
    """The bf16 weight gradient: the LDS-DMA ring where the chunk's pixel rows are whole 64-row K tiles, else the
    register-staged kernel (rt_backward.hip lstm_wgrad)."""
    rows = o["T"] * o["B"] * o["h"] * o["w"]
    if rows % 64 == 0:
        return "LDS-DMA" in o["wvar"] and "gemm_pipe" in o["wvar"] and "+GIm2colT]" in o["wvar"]
    return "register-staged" in o["wvar"] and "LdIm2colTB" in o["wvar"] and "split products" not in o["wvar"]


@pytest.mark.parametrize("sel", sorted(SELECT))
@pytest.mark.parametrize("case", C.UNROLL_CASES, ids=C.case_id)
def test_convlstm_bf16_on_own_operands(cuda, monkeypatch, case, sel):
    """Frame-resident, paired and per-step forward and BPTT on the grids one workgroup holds: every step's gates,
    c_t, h_t, dZ_t, dx_t, and dh0, dc0, the weight and bias gradients."""
    fw, bw = SELECT[sel]
    o = _learner(cuda, monkeypatch, case, {"AAA_FRAMES_FWD": fw, "AAA_FRAMES_BWD": bw})
    fv, bv = o["fvar"], o["bvar"]
    if fw == "0":
        assert _steps(fv), fv
    else:
        assert "bf16 frame-resident [x|h] recurrence" in fv and f"{fw} WG per frame" in fv, fv
    if bw == "0":
        assert "bf16 dh dgrad + fused gate bwd" in bv and "EpiConvLstmBwd" in bv, bv
        assert "batched dx" in o["xvar"] and "EpiStoreBiasT" in o["xvar"], o["xvar"]
        assert o["mask"] == 0, o["mask"]
    else:
        kern = "k_convlstm_bwd_frames<0, false" if bw == "1" else "k_convlstm_bwd_pairs"
        assert "bf16 frame-resident BPTT + dx" in bv and f"{bw} WG per frame" in bv and kern in bv, bv
        assert o["mask"] == N.CQM_C | N.CQM_G | N.CQM_DO, o["mask"]
    assert _wgrad_variant_ok(o), o["wvar"]
    if case == (4, 3, 64, 64, False):
        assert "LDS-DMA" in o["wvar"], o["wvar"]   # 768 pixel rows: the ring
    _check(o, f"{sel} {C.case_id(case)}")


@pytest.mark.parametrize("band", ["1", "0"])
@pytest.mark.parametrize("case", C.BAND_CASES, ids=C.case_id)
def test_convlstm_bf16_band_mode_on_own_operands(cuda, monkeypatch, case, band):
    """The 21x21 grid: band mode (four bands of 5, 5, 5, 6 rows exchanging halo rows of h_t and dZ_t through
    memory), and the per-step launches on the same grid (AAA_FRAMES_BAND = 0)."""
    o = _learner(cuda, monkeypatch, case, {} if band == "1" else {"AAA_FRAMES_BAND": "0"})
    if band == "1":
        assert "band-mode" in o["fvar"] and "4 bands per frame" in o["fvar"], o["fvar"]
        assert "band-mode" in o["bvar"] and "k_convlstm_bwd_frames<0, true" in o["bvar"], o["bvar"]
        assert o["mask"] == N.CQM_C | N.CQM_G | N.CQM_DO, o["mask"]
    else:
        assert _steps(o["fvar"]), o["fvar"]
        assert "bf16 dh dgrad + fused gate bwd" in o["bvar"] and "EpiConvLstmBwd" in o["bvar"], o["bvar"]
        assert o["mask"] == 0, o["mask"]
    assert _wgrad_variant_ok(o), o["wvar"]
    _check(o, f"band={band} {C.case_id(case)}")


@pytest.mark.parametrize("case", C.WGRAD_EDGE_CASES, ids=C.case_id)
def test_wgrad_bf16_k_loop_edges(cuda, monkeypatch, case):
    """The bf16 weight gradient at 75, 363 and 540 pixel rows (tests/test_gpu_wgrad_paired.py CASES): K tails,
    splits of one or two tiles, image-row ends in the gather -- (a) on gWx, gWh from the stored dZ and [x | h]."""
    o = _learner(cuda, monkeypatch, case, {})
    assert o["T"] * o["B"] * o["h"] * o["w"] in (75, 363, 540)
    assert _wgrad_variant_ok(o), o["wvar"]
    rep = _check(o, f"wgrad edge {C.case_id(case)}", wgrad_only=True)
    assert set(rep) == {"gWx", "gWh"}


def _cell_gate_dtype(B, h, w):
    """The cell entry's gate storage type: gates_f16(dtype, M) (csrc/rt.h), the same rule as a learner's of the
    same M = B*h*w -- asked through aaa_core_layout for frames whose grid is (h, w)."""
    cfg = N.Cfg(B, 1, 8 * h - 6, 8 * w - 6, 4, 18, N.BF16, 0)
    assert N.grid(cfg.H, cfg.W) == (h, w)
    ge, mask = ctypes.c_int(), ctypes.c_int()
    N.check(N.load().aaa_core_layout(ctypes.byref(cfg), ctypes.byref(ge), ctypes.byref(mask)), "core_layout")
    return torch.float16 if ge.value == 2 else torch.float32


@pytest.mark.parametrize("B,h,w", C.CELL_CASES)
def test_cell_entry_bf16_on_known_inputs(cuda, B, h, w):
    """aaa_convlstm_cell_fwd / _bwd, bf16, on f32_split_ref.CELL_CASES.  From the code (rt_components.hip
    cell_fwd_impl / cell_bwd_impl): the entry takes fp32 x, h0, c0, dh1, dc1; it rounds x and h0 to bf16 itself
    (cell_xh) and reads c0, dh1, dc1 as fp32.  It hands back h1 in fp32, NOT rounded (EpiConvLstmFwd's hout),
    c1 fp32, and dx, dh0, dc0 and the twelve gradients fp32; its gates (fp16) and dZ (bf16) stay in its
    workspace, so the reference rounds its own (convlstm_bf16_ref.cell_ref) and the gates are 4 e_flip + 1e-5."""
    io = C.cell_inputs(B, h, w)
    M = B * h * w
    r = CellRunner(B, h, w, "bf16", cuda)
    flat = torch.cat([torch.from_numpy(PARAMS[k]).reshape(-1) for k in PARAMS if k.startswith(R.LSTM)]).to(cuda)
    packed = r.pack(flat)
    dev = {k: v.to(cuda) for k, v in io.items()}
    N.timing_enable(True)
    try:
        h1, c1, ws = r.forward(packed, dev["x"], dev["h0"], dev["c0"])
        fvar = N.timing_stats(N.TIMER_FWD_STEP)["variant"]
        dx, dh0, dc0, grads = r.backward(packed, ws, dev["dh1"], dev["dc1"])
        torch.cuda.synchronize()
    finally:
        N.timing_enable(False)
    assert "bf16 fused [x|h] step" in fvar, fvar
    rows = lambda t: t.cpu().reshape(M, -1)   # noqa: E731
    got = {"h1": rows(h1), "c1": rows(c1), "dx": rows(dx), "dh0": rows(dh0), "dc0": rows(dc0)}
    got.update(R.split_cell_grads(grads))
    ref, gate = C.cell_ref(io, B, h, w, got["c1"], _cell_gate_dtype(B, h, w))
    bad = []
    for obs in ("h1", "c1", "dx", "dh0", "dc0", "gWx", "gWh", "gb"):
        ratio = V.rel(got[obs], ref[obs]) / gate[obs]
        print(f"[bf16lstm] cell {B}x{h}x{w} {obs}: err/gate {ratio:.3e} (gate {gate[obs]:.2e})")
        if not ratio <= 1.0:
            bad.append((obs, ratio))
    assert not bad, bad
    assert N.pair_status(clear=True) == 0
