"""CPU-side checks of AAA_FLAG_BF16_RESETS (include/aaa.h): the flag's value, what
it adds to the workspace layout -- one region, AAA_BF16_WS_HR, behind every other
-- and that nothing else of the layout moves; and what a mask still cannot go
with.  Layout queries and refused calls only: a call the library accepts would
dereference its addresses, so none is made here (no GPU needed)."""
import ctypes

import pytest

from helpers import ROOT  # noqa: F401  (path setup)

import attention  # noqa: F401
from aaa_amd import _native as N

P = 4096   # a dummy aligned address, never dereferenced: every refusal comes before the device
E_ARG, E_ALIGN = -1, -2
SHAPES = [(2, 3, 84, 84), (256, 20, 84, 84), (5, 3, 168, 168)]   # B, T, H, W
REGIONS = range(0, 30)


def _cfg(B=2, T=3, H=84, W=84, dtype=N.BF16, flags=0):
    return N.Cfg(B, T, H, W, 4, 18, dtype, flags)


def _bytes(cfg):
    lib = N.load()
    return lib.aaa_workspace_bytes(ctypes.byref(cfg)), lib.aaa_packed_bytes(ctypes.byref(cfg))


def _region(cfg, region):
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    rc = N.load().aaa_workspace_region(ctypes.byref(cfg), region, ctypes.byref(off), ctypes.byref(nb))
    return rc, off.value, nb.value


def _layout(cfg):
    ge, mask = ctypes.c_int(), ctypes.c_int()
    rc = N.load().aaa_core_layout(ctypes.byref(cfg), ctypes.byref(ge), ctypes.byref(mask))
    return rc, ge.value, mask.value


def _call(name, cfg, phases, reset):
    lib = N.load()
    io = N.IO(*[P] * len(N.IO_FIELDS))
    rc = getattr(lib, name)(ctypes.byref(cfg), ctypes.byref(io), phases, reset, None)
    return rc, lib.aaa_last_error()


def test_flag_value_and_abi():
    assert N.FLAG_BF16_RESETS == 16 and N.BF16_WS_HR == 30
    assert N.load().aaa_abi_version() == 12   # additive: no bump
    for dtype in (N.BF16, N.F32):
        assert _bytes(_cfg(dtype=dtype, flags=16))[0] > 0
        assert _bytes(_cfg(dtype=dtype, flags=8)) == (0, 0)        # 8 is still no flag
        assert _bytes(_cfg(dtype=dtype, flags=16 | 8)) == (0, 0)
        assert _bytes(_cfg(dtype=dtype, flags=32)) == (0, 0)


@pytest.mark.parametrize("B,T,H,W", SHAPES)
@pytest.mark.parametrize("other", [0, N.FLAG_STATEFUL_CORE, N.FLAG_FRAMES_U8, N.FLAG_STATEFUL_CORE | N.FLAG_FRAMES_U8])
def test_workspace_grows_by_the_hr_region_alone(B, T, H, W, other):
    plain, flagged = _cfg(B, T, H, W, flags=other), _cfg(B, T, H, W, flags=other | N.FLAG_BF16_RESETS)
    h, w = N.grid(H, W)
    bare = T * B * h * w * 128 * 2
    rc, off, nb = _region(flagged, N.BF16_WS_HR)
    assert rc == 0 and nb == bare
    (ws0, pk0), (ws1, pk1) = _bytes(plain), _bytes(flagged)
    assert ws0 > 0 and pk0 == pk1
    assert ws1 - ws0 == (bare + 255) // 256 * 256 == nb    # rows of 256 B: the rounding adds nothing
    # behind every other region, 256-byte aligned, and the last bytes of the workspace
    assert off % 256 == 0 and off == ws0 and off + nb == ws1
    for r in REGIONS:
        a, b = _region(plain, r), _region(flagged, r)
        assert a == b, r
        if a[0] == 0:
            assert a[1] + a[2] <= off, r
    assert _layout(plain) == _layout(flagged) and _layout(plain)[0] == 0


@pytest.mark.parametrize("B,T,H,W", SHAPES)
def test_region_30_needs_the_flag_and_bf16(B, T, H, W):
    lib = N.load()
    for cfg in (_cfg(B, T, H, W), _cfg(B, T, H, W, dtype=N.F32), _cfg(B, T, H, W, dtype=N.F32, flags=N.FLAG_BF16_RESETS)):
        rc, _, _ = _region(cfg, N.BF16_WS_HR)
        assert rc == E_ARG and b"region 30" in lib.aaa_last_error()
    # fp32: the flag is accepted and changes nothing
    a, b = _cfg(B, T, H, W, dtype=N.F32), _cfg(B, T, H, W, dtype=N.F32, flags=N.FLAG_BF16_RESETS)
    assert _bytes(a) == _bytes(b) and _bytes(a)[0] > 0
    for r in REGIONS:
        assert _region(a, r) == _region(b, r), r
    assert _layout(a) == _layout(b)


@pytest.mark.parametrize("name,phases", [("aaa_forward_resets", N.FWD_ALL), ("aaa_backward_resets", N.BWD_ALL)])
def test_unflagged_bf16_still_refuses_a_mask(name, phases):
    rc, msg = _call(name, _cfg(), phases, P)
    assert rc == E_ARG and b"fp32" in msg and b"mask" in msg and b"AAA_FLAG_BF16_RESETS" in msg, (rc, msg)


@pytest.mark.parametrize("name,phases", [("aaa_forward_resets", N.FWD_ALL), ("aaa_backward_resets", N.BWD_ALL)])
@pytest.mark.parametrize("off", [4, 8, 12])
def test_flagged_bf16_refuses_a_misaligned_mask(name, phases, off):
    rc, msg = _call(name, _cfg(flags=N.FLAG_BF16_RESETS), phases, P + off)
    assert rc == E_ALIGN and b"16-byte aligned" in msg and b"reset" in msg, (rc, msg)


@pytest.mark.parametrize("other", [0, N.FLAG_STATEFUL_CORE])
def test_flagged_bf16_refuses_a_mask_without_the_core_phase(other):
    rc, msg = _call("aaa_forward_resets", _cfg(flags=N.FLAG_BF16_RESETS | other), N.FWD_VISION | N.FWD_TAIL, P)
    assert rc == E_ARG and b"AAA_FWD_CORE" in msg, (rc, msg)
