"""CPU evidence for the bounds of tests/test_gpu_vision_f32_frames.py (the frame-resident fp32
vision encoder forward, csrc/vision_f32.h) and the argument checks of its checker entry
aaa_vision_enc_f32_fwd (include/aaa.h), which need no GPU.

On integer-valued (uint8) frames conv1's input site is invisible -- the frames are exact in bf16,
so cutting x to two bf16 parts changes nothing -- which is why the GPU test bounds conv1.W alone
there; and plain float32 convolution meets e2 / 4 at every other site, so the GPU test's e2 / 2
is a bound the reference arithmetic itself keeps with a factor two to spare.
Reference: attention.py:155-170 on X.transpose(1,3) (:179)."""
import ctypes

import pytest
import torch

import f32_split_ref as R
from helpers import rel_err

import attention  # noqa: F401
from aaa_amd import _native as N

CASES = [(3, 84, 84), (5, 64, 64)]
U8 = N.FLAG_FRAMES_U8
A = 4096   # a dummy aligned address, never dereferenced: every refusal comes before the device


@pytest.mark.parametrize("n,H,W", CASES)
def test_integer_frames_bounds_on_cpu(n, H, W):
    X = R.frames(1, n, H, W)[0]                      # integer-valued, (n,H,W,3)
    x_ref = X.permute(0, 3, 2, 1).contiguous()
    h, w = R.ref_cpu.grid_of(H, W)
    dy2 = torch.zeros(n, 64, w, h)
    W64, W32 = R.cnn_weights(), R.cnn_weights(dtype=torch.float32)
    ex, e2 = R.cnn_e2(W64, x_ref, dy2)
    assert e2["conv1.x", "y1"] == 0.0, e2["conv1.x", "y1"]
    f32 = R.cnn_pieces(W32, x_ref, dy2)
    r1 = rel_err(f32["y1"], ex["y1"]) / e2["conv1.W", "y1"]
    print(f"({n},{H},{W}) float32 conv1: err / e2[conv1.W] {r1:.3f}")
    assert r1 <= 0.25, r1
    # conv2 on the float32 y1 against fp64 on that same y1, as the GPU test evaluates a kernel
    ex2, e22 = R.cnn_e2(W64, x_ref, dy2, y1_in=f32["y1"])
    y2 = R.cnn_pieces(W32, x_ref, dy2, y1_in=f32["y1"])["y2"]
    for s in ("conv2.W", "conv2.y1"):
        r2 = rel_err(y2, ex2["y2"]) / e22[s, "y2"]
        print(f"({n},{H},{W}) float32 conv2: err / e2[{s}] {r2:.3f}")
        assert r2 <= 0.25, (s, r2)


def _fwd(lib, d, ptrs=(A,) * 6):
    return lib.aaa_vision_enc_f32_fwd(ctypes.byref(d) if d is not None else None, *ptrs, None)


REFUSED = {
    "bf16 dtype": N.EncDesc(1, 84, 84, N.BF16, U8, 192),
    "out_ld 56": N.EncDesc(1, 84, 84, N.F32, U8, 56),
    "out_ld 196": N.EncDesc(1, 84, 84, N.F32, U8, 196),
    "N = 0": N.EncDesc(0, 84, 84, N.F32, U8, 192),
    "stateful flag": N.EncDesc(1, 84, 84, N.F32, U8 | N.FLAG_STATEFUL_CORE, 192),
    "frame 4x4": N.EncDesc(1, 4, 4, N.F32, U8, 192),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_enc_f32_entry_refuses_unsupported(what):
    lib = N.load()
    assert _fwd(lib, REFUSED[what]) == -1 and lib.aaa_last_error(), what


def test_enc_f32_entry_refuses_null_and_misaligned():
    lib = N.load()
    assert _fwd(lib, None) == -1 and b"NULL" in lib.aaa_last_error()
    d = N.EncDesc(2, 84, 84, N.F32, U8, 192)
    for i in range(6):   # cnn_params, packed, frames, xp, y1, out
        ptrs = [A] * 6
        ptrs[i] = None
        assert _fwd(lib, d, ptrs) == -1, i
        ptrs[i] = A + 8
        assert _fwd(lib, d, ptrs) == -2, i   # AAA_E_ALIGN


def test_packed_bytes_hold_the_presplit_weights():
    lib = N.load()
    f32 = lib.aaa_vision_cnn_packed_bytes(ctypes.byref(N.CnnDesc(1, 84, 84, N.F32)))
    b16 = lib.aaa_vision_cnn_packed_bytes(ctypes.byref(N.CnnDesc(1, 84, 84, N.BF16)))
    plain = (32 * 256 + 64 * 512 + 4 * 32 * 256)
    assert f32 == plain * 4 + 3 * 2 * (32 * 256 + 64 * 512) and b16 == plain * 2
