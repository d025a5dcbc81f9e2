"""The fp32 path's split-product GEMMs (AAA_F32_SPLIT6: fp32 operands cut into
hi + mid + lo bf16 parts, six part products on the bf16 MFMA) held to fp32
accuracy, kernel by kernel, against fp64 evaluated on the kernel's own inputs:

  a. the ConvLSTM forward: frame-group kernels k_convlstm_fwd_f32ps (G = 8) and
     k_convlstm_fwd_f32<G, ..., true> (G = 4), and the per-step launches'
     split-product tiles (AAA_F32_FRAMES = 0);
  b. the frame-group BPTT + dx k_convlstm_bwd_f32, the per-step dh chain with
     the batched dx, and the GemmCfgS6LK weight gradient;
  c. the cell component entry (aaa_convlstm_cell_fwd / _bwd);
  d. the vision CNN component entry (conv1, conv2, conv2's dgrad, both weight
     gradients).

Bound (f32_split_ref.py): for every operand site s that reaches an observable,
err(kernel, fp64) <= e2[s, observable] / 2, where e2 is the error of the same
fp64 formulas with site s cut to its first two bf16 parts -- what a kernel that
lost a lo part there would show.  test_f32_split_emulation.py shows on the CPU
that plain float32 arithmetic sits within e2 / 4 at every case used here.  What
no GEMM site is bounded on (gates, bias gradients, dc0) stays at the project's
1e-4.  The learner cases read the kernels' inputs from the workspace
(aaa_workspace_region AAA_WS_CORE_XH / _DO / _DX, aaa_core_export) and run the
backward in phases (HEAD, then CORE) so that dO is the kernels' own.

Reference: attention.py:110-126 (ConvLSTMCell.forward) over T steps and :155-170
(vision_cnn), and their autograd backward (main_mp.py:77).

Measured err / e2 (MI355X) and which of these checks catch a zeroed lo plane:
DESIGN.md "fp32 split products: accuracy".
"""
import pytest
import torch

import f32_split_ref as R
from helpers import detinit, rel_err
from oracle import ref_cpu
from test_gpu_parity import RTOL, _agent, _cot

import attention
from aaa_amd.runtime import CellRunner, CnnRunner

pytestmark = pytest.mark.gpu
N = attention._pkg._native
PARAMS = detinit.deterministic_params(0, 18)
_FWD_REF = {}   # case -> (x, exact fp64 recurrence, e2): x_t is the vision encoder's, the same for every G


def _bound(what, got, ref, e2, obs, reach):
    """err(got, ref[obs]) <= e2[s, obs] / 2 for every site s reaching obs; prints err / e2 first."""
    err = rel_err(got, ref[obs])
    sites = [s for s in reach[obs] if (s, obs) in e2]
    assert sites, (what, obs)
    print(f"[f32split] {what} {obs}: err {err:.3e} " + " ".join(f"err/e2[{s}] {err / e2[s, obs]:.3f}" for s in sites))
    return [f"{what} {obs}: err {err:.3e} > e2[{s}] / 2 = {e2[s, obs] / 2:.3e}" for s in sites if not err <= e2[s, obs] / 2]


def _flat(cuda, keys):
    return torch.cat([torch.from_numpy(PARAMS[k]).reshape(-1) for k in keys]).to(cuda)


def _learner(cuda, monkeypatch, case, frames, backward):
    """One forward (and phased backward) of an UnrollRunner; everything read back on the host."""
    T, B, H, W, state = case
    monkeypatch.setenv("AAA_F32_FRAMES", frames)
    h, w = ref_cpu.grid_of(H, W)
    M = B * h * w
    ag = _agent(cuda, grid=(h, w))
    r = ag._runner(B, T, H, W, cuda, False, False)
    S = ag._basis_for(r.h, r.w, H, W, cuda)
    flat, packed = ag._packed_params(r, list(ag.parameters()))
    X = R.frames(T, B, H, W).to(cuda)
    h0 = c0 = None
    if state:
        h0, c0 = (t.to(cuda) for t in R.state_in(B, h, w))
    ws = r.new_workspace()
    o = {"B": B, "h": h, "w": w, "T": T}
    N.timing_enable(True)
    try:
        _, _, _, hT, cT = r.forward(flat, packed, S, X, ws, h0=h0, c0=c0, want_attn=False, want_state=True)
        o["fvar"] = N.timing_stats(N.TIMER_FWD_STEP)["variant"]
        xh = r.workspace_region(ws, N.WS_CORE_XH, (T + 1, M, 192)).cpu()
        core = [torch.empty(s, device=cuda) for s in r.core_shapes(T)]
        r.core_export(ws, 0, T, *core)
        gates, c, hh = (t.cpu() for t in core)
        o["hT"], o["cT"] = hT.cpu().reshape(M, 128), cT.cpu().reshape(M, 128)
        if backward:
            Gl, Gv = (g.to(cuda) for g in _cot(T, B))
            g, _, _ = r.backward(flat, packed, S, X, ws, Gl, Gv, phases=N.BWD_HEAD)
            dO = r.workspace_region(ws, N.WS_CORE_DO, (T, M, 128)).cpu()
            dhT, dcT = R.state_cot(B, h, w, float(dO.abs().max()))   # at the scale of the readout's cotangent
            g, dh0, dc0 = r.backward(flat, packed, S, X, ws, Gl, Gv, dhT=dhT.to(cuda), dcT=dcT.to(cuda), grads=g,
                                     want_state_grads=True, phases=N.BWD_CORE)
            o["bvar"] = N.timing_stats(N.TIMER_BPTT_STEP)["variant"]
            o["wvar"] = N.timing_stats(N.TIMER_CORE_WGRAD)["variant"]
            dx = r.workspace_region(ws, N.WS_CORE_DX, (T, M, 64)).cpu()
            lstm = g[r.offsets[4]:r.offsets[16]]   # the 12 ConvLSTM tensors, state_dict order
            assert lstm.numel() == 4 * (128 * 64 * 9 + 128 + 128 * 128 * 9)
            o["grads"] = R.split_cell_grads(lstm)
            o.update(dO=R.to_ref(dO, B, h, w), dx=R.to_ref(dx, B, h, w), dh0=R.to_ref(dh0.cpu().reshape(M, 128), B, h, w),
                     dc0=R.to_ref(dc0.cpu().reshape(M, 128), B, h, w),
                     dhT=R.to_ref(dhT.reshape(M, 128), B, h, w), dcT=R.to_ref(dcT.reshape(M, 128), B, h, w))
    finally:
        N.timing_enable(False)
    o["x"] = R.to_ref(xh[:T, :, :64].contiguous(), B, h, w)
    o["hprev"] = R.to_ref(xh[:T, :, 64:].contiguous(), B, h, w)       # slot t's h half: h_{t-1}, slot 0 the incoming h0
    o["h0"] = None if h0 is None else o["hprev"][0]
    o["c0"] = None if c0 is None else R.to_ref(c0.cpu().reshape(M, 128), B, h, w)
    o["gates"], o["c"], o["hs"] = R.gates_to_ref(gates, B, h, w), R.to_ref(c, B, h, w), R.to_ref(hh, B, h, w)
    return o


def _fwd_variant_ok(var, frames):
    if frames == "8":
        return "k_convlstm_fwd_f32ps" in var and "8 WG per frame" in var
    if frames == "4":
        return "k_convlstm_fwd_f32<" in var and "4 WG per frame" in var and "split products" in var
    return "WG per frame" not in var and var.startswith("fp32") and "step" in var


@pytest.mark.parametrize("frames", ["8", "4", "0"])
@pytest.mark.parametrize("case", R.UNROLL_CASES, ids=lambda c: "T{}B{}_{}x{}{}".format(*c[:4], "_state" if c[4] else ""))
def test_convlstm_forward_fp32_accuracy(cuda, monkeypatch, case, frames):
    """a.  h_t and c_t of every step, free-running in fp64 from the kernel's own x_t (and h0 / c0)."""
    o = _learner(cuda, monkeypatch, case, frames, backward=False)
    assert _fwd_variant_ok(o["fvar"], frames), o["fvar"]
    cached = _FWD_REF.get(case)
    if cached is None or not torch.equal(cached[0], o["x"]):
        cached = _FWD_REF[case] = (o["x"],) + R.fwd_e2(R.cell_weights(PARAMS), o["x"], o["h0"], o["c0"])
    _, ex, e2 = cached
    what = f"fwd frames={frames} T={case[0]} B={case[1]} {case[2]}x{case[3]}{' state' if case[4] else ''}"
    if case[4]:
        assert torch.equal(R.from_ref(o["h0"]), R.state_in(o["B"], o["h"], o["w"])[0].reshape(-1, 128))
    bad = _bound(what, o["hs"], ex, e2, "h", R.FWD_REACH) + _bound(what, o["c"], ex, e2, "c", R.FWD_REACH)
    assert rel_err(o["gates"], ex["gates"]) <= RTOL, what
    # the slots the next step and the weight gradient read, and the state handed back, are that h_t / c_t
    assert torch.equal(o["hprev"][1:], o["hs"][:-1]), what + ": XH slot t+1 is not h_t"
    assert torch.equal(o["hT"], R.from_ref(o["hs"][-1])) and torch.equal(o["cT"], R.from_ref(o["c"][-1])), what
    assert not bad, bad
    assert N.pair_status(clear=True) == 0


def _check_backward(what, o, sites, bounded):
    W64 = R.cell_weights(PARAMS)
    cprev = torch.cat([(torch.zeros_like(o["c"][0]) if o["c0"] is None else o["c0"])[None], o["c"][:-1]])
    ex, e2 = R.bwd_e2(W64, o["x"], o["hprev"], o["gates"], cprev, o["c"], o["dO"], o["dhT"], o["dcT"], sites=sites)
    got = {"dx": o["dx"], "dh0": o["dh0"], "gWx": o["grads"]["gWx"], "gWh": o["grads"]["gWh"]}
    bad = []
    for obs in bounded:
        bad += _bound(what, got[obs], ex, e2, obs, R.BWD_REACH)
    for obs, t in (("dx", o["dx"]), ("dh0", o["dh0"]), ("dc0", o["dc0"]), ("gb", o["grads"]["gb"]),
                   ("gWx", got["gWx"]), ("gWh", got["gWh"])):
        assert rel_err(t, ex[obs]) <= RTOL, (what, obs, rel_err(t, ex[obs]))
    assert not bad, bad


@pytest.mark.parametrize("frames", ["8", "0"])
@pytest.mark.parametrize("case", R.UNROLL_CASES, ids=lambda c: "T{}B{}_{}x{}{}".format(*c[:4], "_state" if c[4] else ""))
def test_convlstm_backward_fp32_accuracy(cuda, monkeypatch, case, frames):
    """b.  BPTT in fp64 from the same run's exported gates, c_t, h_t, x_t and dO_t, with carried dhT / dcT: dx_t
    and dh0 (the dgrad's sites), the eight weight gradients (the wgrad's), on the frame-group BPTT + dx (8) and on
    the per-step dh chain + batched dx (0); the weight gradient is GemmCfgS6LK's in both."""
    o = _learner(cuda, monkeypatch, case, frames, backward=True)
    assert _fwd_variant_ok(o["fvar"], frames), o["fvar"]
    if frames == "8":
        assert "frame-group BPTT + dx (bf16x6 split products)" in o["bvar"], o["bvar"]
    else:
        assert "fp32 dh dgrad + fused gate bwd" in o["bvar"], o["bvar"]
    assert "gemm_kernel_s6l+GemmCfgS6LK" in o["wvar"], o["wvar"]
    what = f"bwd frames={frames} T={case[0]} B={case[1]} {case[2]}x{case[3]}{' state' if case[4] else ''}"
    _check_backward(what, o, R.DGRAD_SITES + R.WGRAD_SITES, ("dx", "dh0", "gWx", "gWh"))
    assert N.pair_status(clear=True) == 0


@pytest.mark.parametrize("case", R.WGRAD_EDGE_CASES, ids=lambda c: "T{}B{}_{}x{}".format(*c[:4]))
def test_wgrad_k_loop_edges_fp32_accuracy(cuda, monkeypatch, case):
    """b.  The weight gradient's K-loop edges (test_gpu_wgrad_paired.CASES) at 75, 363 and 540 pixel rows: odd
    tile counts within the splits, 18 splits of one or two tiles with a K tail, image-row ends in the gather."""
    o = _learner(cuda, monkeypatch, case, "0", backward=True)
    assert "gemm_kernel_s6l+GemmCfgS6LK" in o["wvar"], o["wvar"]
    rows = o["T"] * o["B"] * o["h"] * o["w"]
    assert rows in (75, 363, 540)
    _check_backward(f"wgrad edge {rows} rows", o, R.WGRAD_SITES, ("gWx", "gWh"))
    assert N.pair_status(clear=True) == 0


@pytest.mark.parametrize("B,h,w", R.CELL_CASES)
def test_cell_entry_fp32_accuracy(cuda, B, h, w):
    """c.  aaa_convlstm_cell_fwd / _bwd on random x, h0, c0, dh1, dc1: the B = 1 / small-batch fused step tiles
    and the weight gradient with no learner around them."""
    c = R.cell_case(B, h, w)
    M = B * h * w
    r = CellRunner(B, h, w, "fp32", cuda)
    packed = r.pack(_flat(cuda, [k for k in PARAMS if k.startswith(R.LSTM)]))
    io = {k: v.to(cuda) for k, v in c["io"].items()}
    N.timing_enable(True)
    try:
        h1, c1, ws = r.forward(packed, io["x"], io["h0"], io["c0"])
        fvar = N.timing_stats(N.TIMER_FWD_STEP)["variant"]
        dx, dh0, dc0, grads = r.backward(packed, ws, io["dh1"], io["dc1"])
        wvar = N.timing_stats(N.TIMER_CORE_WGRAD)["variant"]
        torch.cuda.synchronize()
    finally:
        N.timing_enable(False)
    assert "fp32 fused [x|h] step" in fvar, fvar
    assert "gemm_kernel_s6l+GemmCfgS6LK" in wvar, wvar
    ref = lambda t: R.to_ref(t.cpu().reshape(M, -1), B, h, w)   # noqa: E731
    what = f"cell {B}x{h}x{w}"
    bad = _bound(what, ref(h1)[None], c["fwd64"], c["fwd_e2"], "h", R.FWD_REACH)
    bad += _bound(what, ref(c1)[None], c["fwd64"], c["fwd_e2"], "c", R.FWD_REACH)
    g = R.split_cell_grads(grads)
    got = {"dx": ref(dx)[None], "dh0": ref(dh0), "gWx": g["gWx"], "gWh": g["gWh"]}
    for obs in ("dx", "dh0", "gWx", "gWh"):
        bad += _bound(what, got[obs], c["bwd64"], c["bwd_e2"], obs, R.BWD_REACH)
    assert rel_err(ref(dc0), c["bwd64"]["dc0"]) <= RTOL and rel_err(g["gb"], c["bwd64"]["gb"]) <= RTOL, what
    assert not bad, bad
    assert N.pair_status(clear=True) == 0


@pytest.mark.parametrize("N_,H,W", R.CNN_CASES)
def test_vision_cnn_entry_fp32_accuracy(cuda, monkeypatch, N_, H, W):
    """d.  aaa_vision_cnn_fwd / _bwd on scaled frames (x 0.37: integer frames are exact in bf16, conv1's input
    site would be invisible): y1, y2, dy1, gW1, gW2.  conv2's reference reads the kernel's own y1, gW1's the
    kernel's own dy1.  The entry records no timer variant; that the split-product kernels are what ran is shown by
    the run differing in bits from one with AAA_F32_SPLIT6=0 (the fp32 MFMA), which is held to the same bounds."""
    c = R.cnn_case(N_, H, W)
    keys = [k for k in PARAMS if k.startswith(R.CNN)]
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("AAA_F32_SPLIT6", mode)
        r = CnnRunner(N_, H, W, "fp32", cuda)
        flat = _flat(cuda, keys)
        packed = r.pack(flat)
        y2, y1, ws = r.forward(flat, packed, c["X"].to(cuda), want_y1=True)
        grads, dy1 = r.backward(packed, ws, c["dy2"].to(cuda), want_dy1=True)
        torch.cuda.synchronize()
        outs[mode] = [t.cpu() for t in (y1, y2, dy1, grads)]
    assert not any(torch.equal(a, b) for a, b in zip(outs["1"], outs["0"])), "AAA_F32_SPLIT6 selected no other kernel"
    W64 = R.cnn_weights(PARAMS)
    for mode in ("1", "0"):
        y1, y2, dy1, grads = outs[mode]
        nhwc = lambda t: t.permute(0, 3, 2, 1).contiguous()   # noqa: E731
        ex, e2 = R.cnn_e2(W64, c["x_ref"], c["dy2_ref"], y1_in=nhwc(y1), dy1_in=nhwc(dy1))
        n1, n2 = 32 * 3 * 64, 64 * 32 * 16
        got = {"y1": nhwc(y1), "y2": nhwc(y2), "dy1": nhwc(dy1), "gW1": grads[:n1].reshape(32, 3, 8, 8),
               "gW2": grads[n1 + 32:n1 + 32 + n2].reshape(64, 32, 4, 4)}
        what = f"cnn {N_}x{H}x{W} split6={mode}"
        bad = []
        for obs in R.CNN_REACH:
            bad += _bound(what, got[obs], ex, e2, obs, R.CNN_REACH)
        assert rel_err(grads[n1:n1 + 32], ex["gb1"]) <= RTOL and rel_err(grads[n1 + 32 + n2:], ex["gb2"]) <= RTOL, what
        assert not bad, bad
    assert N.pair_status(clear=True) == 0
