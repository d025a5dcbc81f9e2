"""CPU-side checks of the bf16 encoder checker entries (aaa_vision_enc_*,
include/aaa.h): the workspace query accepts what the learner's encoder runs
and returns 0 for what the entries refuse, and both entries refuse a NULL
desc, an fp32 desc, a short or odd output pitch, unknown flags, NULL buffers
and misaligned pointers before any device call (no GPU needed)."""
import ctypes

import pytest

from helpers import ROOT  # noqa: F401  (path setup)

import attention  # noqa: F401
from aaa_amd import _native as N

U8 = N.FLAG_FRAMES_U8
ACCEPTED = [N.EncDesc(1, 84, 84, N.BF16, U8, 192), N.EncDesc(70, 80, 80, N.BF16, U8, 64),
            N.EncDesc(2, 168, 168, N.BF16, 0, 192), N.EncDesc(3, 20, 24, N.BF16, 0, 72)]
REFUSED = {
    "fp32 dtype": N.EncDesc(1, 84, 84, N.F32, U8, 192),
    "out_ld 56": N.EncDesc(1, 84, 84, N.BF16, U8, 56),
    "out_ld 196": N.EncDesc(1, 84, 84, N.BF16, U8, 196),
    "N = 0": N.EncDesc(0, 84, 84, N.BF16, U8, 192),
    "stateful flag": N.EncDesc(1, 84, 84, N.BF16, U8 | N.FLAG_STATEFUL_CORE, 192),
    "frame 4x4": N.EncDesc(1, 4, 4, N.BF16, U8, 192),
}
A = 4096   # a dummy aligned address, never dereferenced: every refusal comes before the device


def _fwd(lib, d, ptrs=(A,) * 6):
    return lib.aaa_vision_enc_fwd(ctypes.byref(d) if d is not None else None, *ptrs, None)


def _bwd(lib, d, ptrs=(A,) * 7, ws=A):
    return lib.aaa_vision_enc_bwd(ctypes.byref(d) if d is not None else None, *ptrs, None, ws, None)


def test_enc_workspace_query_accepts_supported():
    lib = N.load()
    sizes = [lib.aaa_vision_enc_workspace_bytes(ctypes.byref(d)) for d in ACCEPTED]
    # the two packed-gradient accumulators and at least one workgroup's partials
    assert all(s >= (32 * 256 + 64 * 512) * 4 + (64 * 512 + 32 * 256 + 32) * 4 for s in sizes), sizes
    assert sizes[1] > sizes[0]   # one partial per eight frames
    # the packed weights come from aaa_vision_cnn_pack with a bf16 desc of the same frames
    assert lib.aaa_vision_cnn_packed_bytes(ctypes.byref(N.CnnDesc(1, 84, 84, N.BF16))) > 0


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_enc_entries_refuse_unsupported(what):
    lib = N.load()
    d = REFUSED[what]
    assert lib.aaa_vision_enc_workspace_bytes(ctypes.byref(d)) == 0, what
    assert _fwd(lib, d) == -1 and lib.aaa_last_error(), what
    assert _bwd(lib, d) == -1 and lib.aaa_last_error(), what


def test_enc_entries_refuse_null_desc_and_buffers():
    lib = N.load()
    assert lib.aaa_vision_enc_workspace_bytes(None) == 0
    assert _fwd(lib, None) == -1 and b"NULL" in lib.aaa_last_error()
    assert _bwd(lib, None) == -1 and b"NULL" in lib.aaa_last_error()
    d = ACCEPTED[0]
    for i in range(6):   # cnn_params, packed, frames, xp, y1, out
        ptrs = [A] * 6
        ptrs[i] = None
        assert _fwd(lib, d, ptrs) == -1, i
    for i in range(7):   # packed, frames, dy2, y1, xp, dy1, cnn_grads
        ptrs = [A] * 7
        ptrs[i] = None
        assert _bwd(lib, d, ptrs) == -1, i
    assert _bwd(lib, d, ws=None) == -1


def test_enc_entries_refuse_misaligned_pointers():
    lib = N.load()
    d = ACCEPTED[0]
    for i in range(6):
        ptrs = [A] * 6
        ptrs[i] = A + 8
        assert _fwd(lib, d, ptrs) == -2, i   # AAA_E_ALIGN
    for i in range(7):
        ptrs = [A] * 7
        ptrs[i] = A + 2
        assert _bwd(lib, d, ptrs) == -2, i
    assert _bwd(lib, d, ws=A + 4) == -2
