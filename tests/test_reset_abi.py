"""CPU-side checks of the episode-start entries (aaa_forward_resets /
aaa_backward_resets, include/aaa.h): both symbols are exported and bound, and
what a mask cannot go with -- a bf16 cfg, a forward phase mask without
AAA_FWD_CORE, a mask that is not 16-byte aligned -- is refused with a message
before any device call (no GPU needed; the addresses are dummies)."""
import ctypes

import pytest

from helpers import ROOT  # noqa: F401  (path setup)

import attention  # noqa: F401
from aaa_amd import _native as N

P = 4096   # a dummy aligned address, never dereferenced: every refusal comes before the device
E_ARG, E_ALIGN = -1, -2


def _cfg(dtype=N.F32, flags=0):
    return N.Cfg(2, 3, 84, 84, 4, 18, dtype, flags)


def _io():
    return N.IO(*[P] * len(N.IO_FIELDS))


def _fwd(cfg, phases, reset):
    lib = N.load()
    io = _io()
    rc = lib.aaa_forward_resets(ctypes.byref(cfg), ctypes.byref(io), phases, reset, None)
    return rc, lib.aaa_last_error()


def _bwd(cfg, phases, reset):
    lib = N.load()
    io = _io()
    rc = lib.aaa_backward_resets(ctypes.byref(cfg), ctypes.byref(io), phases, reset, None)
    return rc, lib.aaa_last_error()


def test_symbols_are_exported_and_bound():
    for name in ("aaa_forward_resets", "aaa_backward_resets"):
        assert name in N.EXPORTS
        assert hasattr(N.load(), name)
    assert N.load().aaa_abi_version() == 12   # additive: no bump


@pytest.mark.parametrize("call,phases", [(_fwd, N.FWD_ALL), (_bwd, N.BWD_ALL)], ids=["forward", "backward"])
def test_refuses_bf16_with_a_mask(call, phases):
    rc, msg = call(_cfg(N.BF16), phases, P)
    assert rc == E_ARG and b"fp32" in msg and b"mask" in msg, (rc, msg)


@pytest.mark.parametrize("flags", [0, N.FLAG_STATEFUL_CORE])
def test_refuses_a_mask_without_the_core_phase(flags):
    rc, msg = _fwd(_cfg(flags=flags), N.FWD_VISION | N.FWD_TAIL, P)
    assert rc == E_ARG and b"AAA_FWD_CORE" in msg, (rc, msg)


@pytest.mark.parametrize("call,phases", [(_fwd, N.FWD_ALL), (_bwd, N.BWD_ALL)], ids=["forward", "backward"])
@pytest.mark.parametrize("off", [4, 8, 12])
def test_refuses_a_misaligned_mask(call, phases, off):
    rc, msg = call(_cfg(), phases, P + off)
    assert rc == E_ALIGN and b"16-byte aligned" in msg and b"reset" in msg, (rc, msg)
