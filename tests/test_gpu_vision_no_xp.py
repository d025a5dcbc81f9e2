"""The learner's forward stores no bordered frame image (Xp) where a frame-resident
vision encoder runs (csrc/rt_forward.hip vision_fwd: k_vision_fwd_f32 / k_vision_fwd
with resident_xp = false), and the backward never reads one where such a forward can
run (csrc/rt.h vis_frames_layout): the fused backward rebuilds the image in LDS as
before, the layered launches rebuild it from the observation (csrc/rt_backward.hip
conv1_wgrad_frames).

Reference: attention.py:153-170 (VisionNetwork.vision_cnn on X.transpose(1,3), :179) and
its autograd backward, through the CPU oracle (oracle/ref_cpu.py) at the existing gates:
1e-4 for fp32, 2e-2 for bf16 against the mask-matched bf16-emulated oracle.

Every run starts from a workspace filled with 0xFF (NaN patterns in fp32 and bf16): a
backward that read a stored Xp the forward never wrote would show NaN in conv1's weight
gradient.  The timers' variants say which kernels ran, so no case compares a path with
itself.

Shapes: T=2, B=2 (F=4 frames, fewer than the CUs: more than one workgroup, each with one
frame) at 84x84 (11x11 grid) and one case at 64x64 (8x8); T=3, B=2 for the chunked vision
backward inside the CORE phase.  AAA_VBWD_MINF=0 lets the fp32 fused backward run below
its one-frame-per-CU floor.

Against the layered forward (AAA_VIS_FRAMES=0: frames_rgbx stores Xp, conv1 reads it)
conv1's weight and bias gradients are held to twice the layered path's own run-to-run
difference (two runs with AAA_VIS_FRAMES=0: split-K atomics) and to 1e-6.  (bf16: that
forward is the banded conv1, which stores Xp as the layered one does.)  Measured on MI355X,
old-vs-old / new-vs-old: fp32 8.5e-8 .. 9.4e-8 / 8.2e-8 .. 8.8e-8 over the five fp32 cases (the
12 K splits' atomics reach an element in another order; the rebuilt image has the bits the
store had), bf16 0 / 0 in most draws and 0 / 1.3e-8 in one (three K splits: the pair of
stored-Xp runs repeated its order, the third run did not -- hence the floor in _vs_stored).
"""
import numpy as np
import pytest
import torch

from helpers import detinit, oracle_masks, rel_err
from test_gpu_parity import RTOL, _compare, _cot, _oracle

import attention

pytestmark = pytest.mark.gpu
N = attention._pkg._native

ENVS = ("AAA_VIS_FRAMES", "AAA_VIS_BWD_FRAMES", "AAA_VBWD_MINF")
FWD = {"fp32": "k_vision_fwd_f32", "bf16": "k_vision_fwd]"}
BWD = {"fp32": "k_vision_bwd_f32", "bf16": "k_vision_bwd_frames"}
CONV1 = ("vision.vision_cnn.0.weight", "vision.vision_cnn.0.bias")
_ORACLE = {}


def _env(monkeypatch, env):
    for k in ENVS:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


class _Case:
    """One agent, runner, packed weights, frames and cotangents; run() is one poisoned-workspace forward + backward."""

    def __init__(self, cuda, dtype, T=2, B=2, H=84, W=84, grid=(11, 11), u8=True):
        self.cuda, self.dtype, self.T, self.B, self.H, self.W = cuda, dtype, T, B, H, W
        self.ag = attention.Agent(18, grid=grid, conv_dtype=dtype)
        detinit.load_into(self.ag, detinit.deterministic_params(0, 18, 4))
        self.ag.to(cuda)
        self.r = self.ag._runner(B, T, H, W, cuda, False, u8)
        self.S = self.ag._basis_for(self.r.h, self.r.w, H, W, cuda)
        self.flat, self.packed = self.ag._packed_params(self.r, list(self.ag.parameters()))
        X = torch.from_numpy(detinit.frames_u8(1234, (T, B, H, W, 3)))
        self.X = (X if u8 else X.float()).to(cuda)
        self.Gl, self.Gv = (g.to(cuda) for g in _cot(T, B))

    def run(self, monkeypatch, fwd_env, bwd_env=None, three_calls=False):
        """-> ((logits, values, attn, grads by name), forward variant, backward variant, ReLU masks)."""
        r, cuda = self.r, self.cuda
        ws = r.new_workspace()
        ws.fill_(0xFF)
        N.timing_enable(True)
        try:
            _env(monkeypatch, fwd_env)
            fwd = r.forward(self.flat, self.packed, self.S, self.X, ws)
            torch.cuda.synchronize()
            fvar = N.timing_stats(N.TIMER_VISION_FWD)["variant"]
            relu = r.relu_masks(ws) if self.dtype == "bf16" else None
            _env(monkeypatch, fwd_env if bwd_env is None else bwd_env)
            if three_calls:
                grads = torch.empty(r.n_params, device=cuda)
                for ph in (N.BWD_HEAD, N.BWD_CORE, N.BWD_VISION):
                    r.backward(self.flat, self.packed, self.S, self.X, ws, self.Gl, self.Gv, grads=grads, phases=ph)
            else:
                grads = r.backward(self.flat, self.packed, self.S, self.X, ws, self.Gl, self.Gv)[0]
            torch.cuda.synchronize()
            bvar = N.timing_stats(N.TIMER_VISION_BWD)["variant"]
        finally:
            N.timing_enable(False)
        assert N.pair_status(clear=True) == 0
        named = list(self.ag.named_parameters())
        assert len(named) == 34
        g = {n: t.view_as(p).cpu() for (n, p), t in zip(named, grads.split([p.numel() for _, p in named]))}
        out = (fwd[0].cpu(), fwd[1].cpu(), fwd[2].cpu(), g)
        for n, t in zip(("logits", "values", "attn"), out[:3]):
            assert bool(torch.isfinite(t).all()), f"{n}: non-finite"
        for n, t in g.items():
            assert bool(torch.isfinite(t).all()), f"grad {n}: non-finite"
        print(f"[no_xp] fwd: {fvar}\n[no_xp] bwd: {bvar}")
        return out, fvar, bvar, relu

    def check(self, out, relu, what):
        """Outputs and all 34 gradients against the oracle at the dtype's gate."""
        T, B, H, W = self.T, self.B, self.H, self.W
        if self.dtype == "bf16":
            ref = _oracle(T, B, conv_mode="bf16", H=H, W=W, masks=oracle_masks([relu], B))
            _compare(out, ref, 2e-2, what)
        else:
            key = (T, B, H, W)
            if key not in _ORACLE:
                _ORACLE[key] = _oracle(T, B, H=H, W=W)
            _compare(out, _ORACLE[key], RTOL, what)


def _conv1(out):
    return np.concatenate([out[3][n].numpy().ravel() for n in CONV1])


def _vs_stored(what, new, old, old2):
    """conv1's weight and bias gradients of ``new`` (rebuilt image) against ``old`` (stored Xp): within twice the
    stored-Xp path's own run-to-run difference and 1e-6.  The run-to-run difference is that of split-K fp32
    atomics; the one pair (old, old2) measures it, and where the pair happens to repeat its order (bf16 here:
    three K splits, the pair is bit-identical in most draws, and a third run then differs by ~1e-8) the sample
    says 0 for a quantity that is not: it is floored at 2^-24, the rounding of one reordered fp32 sum."""
    a, b, b2 = _conv1(new), _conv1(old), _conv1(old2)
    d_old, d_new = rel_err(b2, b), rel_err(a, b)
    print(f"{what}conv1 grads old-vs-old {d_old:.3e}, new-vs-old {d_new:.3e}")
    d_run = max(d_old, 2.0 ** -24)
    assert d_new <= 2 * d_run, what + f"conv1 grads new-vs-old {d_new:.3e} > 2 x old-vs-old {d_run:.3e}"
    assert d_new <= 1e-6, what + f"conv1 grads new-vs-old {d_new:.3e}"


@pytest.mark.parametrize("dtype,B,fused", [("fp32", 2, True), ("bf16", 2, False), ("bf16", 4, True)])
def test_fused_backward_poisoned(cuda, monkeypatch, dtype, B, fused):
    """No Xp from the forward, the frame-resident backward (its partials in the Xp region for fp32) at F=4.
    bf16: one workgroup's partials (164 KB) need 7 frames' dY1 region, so F=4 takes the layered launches
    whatever the floor (rt_backward.hip vbwd_on) -- checked as such, and k_vision_bwd_frames at B=4 (F=8)."""
    c = _Case(cuda, dtype, B=B)
    out, fvar, bvar, relu = c.run(monkeypatch, {"AAA_VBWD_MINF": "0"})
    assert FWD[dtype] in fvar and fvar.endswith(", no Xp"), fvar
    assert (BWD[dtype] in bvar) == fused and ("k_vision_bwd" in bvar) == fused, bvar
    c.check(out, relu, f"no Xp, fused backward {dtype} B={B}: ")


@pytest.mark.parametrize("three_calls", [False, True], ids=["one call", "three calls"])
@pytest.mark.parametrize("dtype,env", [("fp32", {"AAA_VBWD_MINF": "0", "AAA_VIS_BWD_FRAMES": "0"}), ("fp32", {}),
                                       ("bf16", {"AAA_VBWD_MINF": "0", "AAA_VIS_BWD_FRAMES": "0"})],
                         ids=["fp32 bwd_frames=0", "fp32 defaults", "bf16 bwd_frames=0"])
def test_layered_backward_after_resident_forward(cuda, monkeypatch, dtype, env, three_calls):
    """The layered launches after a forward that stored no Xp: the image rebuilt from the observation, in the
    CORE phase's chunk (one call: chunk_vision) and in the VISION phase on its own (three calls)."""
    c = _Case(cuda, dtype)
    out, fvar, bvar, relu = c.run(monkeypatch, env, three_calls=three_calls)
    assert FWD[dtype] in fvar and fvar.endswith(", no Xp"), fvar
    assert "k_vision_bwd" not in bvar and "conv1 wgrad" in bvar, bvar
    what = f"no Xp, layered backward {dtype} {sorted(env)}: "
    c.check(out, relu, what)
    # against the layered forward, which stores Xp
    lay = dict(env, AAA_VIS_FRAMES="0")
    old, fold, bold, _ = c.run(monkeypatch, lay, three_calls=three_calls)
    old2 = c.run(monkeypatch, lay, three_calls=three_calls)[0]
    # (fp32: the layered launches; bf16: the banded conv1, which stores Xp as well)
    assert "k_vision_fwd" not in fold and "no Xp" not in fold and ("layered" in fold or "banded conv1" in fold), fold
    assert "k_vision_bwd" not in bold, bold
    _vs_stored(what, out, old, old2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_env_changed_between_the_calls(cuda, monkeypatch, dtype):
    """Forward with AAA_VIS_BWD_FRAMES=1, backward with 0, on one workspace: a decision cached at the forward
    (this backward will be fused, so nobody needs Xp) would leave the layered launches a poisoned image."""
    c = _Case(cuda, dtype)
    on = {"AAA_VBWD_MINF": "0", "AAA_VIS_BWD_FRAMES": "1"}
    off = {"AAA_VBWD_MINF": "0", "AAA_VIS_BWD_FRAMES": "0"}
    out, fvar, bvar, relu = c.run(monkeypatch, on, off)
    assert FWD[dtype] in fvar and fvar.endswith(", no Xp"), fvar
    assert "k_vision_bwd" not in bvar and "conv1 wgrad" in bvar, bvar
    what = f"env changed between the calls {dtype}: "
    c.check(out, relu, what)
    lay = dict(off, AAA_VIS_FRAMES="0")
    old = c.run(monkeypatch, lay)[0]
    old2 = c.run(monkeypatch, lay)[0]
    _vs_stored(what, out, old, old2)


def test_fp32_frames(cuda, monkeypatch):
    """fp32 observations on the fp32 path: the forward skips Xp, the fused backward is uint8-only, so the
    layered launches rebuild the image from fp32 frames."""
    c = _Case(cuda, "fp32", u8=False)
    out, fvar, bvar, relu = c.run(monkeypatch, {"AAA_VBWD_MINF": "0"})
    assert FWD["fp32"] in fvar and fvar.endswith(", no Xp"), fvar
    assert "k_vision_bwd" not in bvar and "conv1 wgrad" in bvar, bvar
    c.check(out, relu, "no Xp, fp32 frames: ")


def test_64x64(cuda, monkeypatch):
    """The 8x8 grid of the fp32 phase tests: 66x66 bordered image, 15x15 conv1 map (a ragged last column block)."""
    c = _Case(cuda, "fp32", H=64, W=64, grid=(8, 8))
    for env, fused in (({"AAA_VBWD_MINF": "0"}, True), ({}, False)):
        out, fvar, bvar, relu = c.run(monkeypatch, env)
        assert FWD["fp32"] in fvar and fvar.endswith(", no Xp"), fvar
        assert (BWD["fp32"] in bvar) == fused, bvar
        c.check(out, relu, f"no Xp, 64x64, fused backward {fused}: ")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_chunked_vision_in_one_backward_call(cuda, monkeypatch, dtype):
    """CORE + VISION in one backward call (the default phases): the vision backward runs per chunk of steps
    (chunk_vision), layered here, each chunk rebuilding its own frames' image; T=3, B=2."""
    c = _Case(cuda, dtype, T=3)
    out, fvar, bvar, relu = c.run(monkeypatch, {"AAA_VBWD_MINF": "0", "AAA_VIS_BWD_FRAMES": "0"})
    assert FWD[dtype] in fvar and fvar.endswith(", no Xp"), fvar
    assert "k_vision_bwd" not in bvar and "conv1 wgrad" in bvar, bvar
    c.check(out, relu, f"no Xp, chunked vision T=3 B=2 {dtype}: ")
