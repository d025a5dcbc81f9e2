"""CPU-side checks of the V-trace loss entry (aaa_vtrace, include/aaa.h): the
symbol is exported and bound, and every argument it refuses -- NULL desc or
io, a NULL required pointer, T < 1, B < 1, A < 2, value_col outside [0, A),
gamma or lambda outside [0, 1], a non-positive or non-finite clip, a negative
or non-finite cost or scale, misaligned dlogits / dvalues -- is refused with
a message before any device call (no GPU needed; the addresses are dummies)."""
import ctypes
import math

import pytest

from helpers import ROOT  # noqa: F401  (path setup)

import attention  # noqa: F401
from aaa_amd import _native as N

P = 4096   # a dummy aligned address, never dereferenced: every refusal comes before the device
REQUIRED = ("logits", "values", "actions", "rewards", "dlogits", "dvalues")
OPTIONAL = ("behaviour_logp", "done", "bootstrap", "vs", "pg_adv", "loss")


def _desc(**kw):
    d = dict(T=4, B=2, A=18, value_col=0, gamma=0.99, lam=1.0, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0,
             baseline_cost=0.5, entropy_cost=0.01, scale=1.0)
    d.update(kw)
    return N.VtraceDesc(*[d[n] for n, _ in N.VtraceDesc._fields_])


def _io(**kw):
    io = N.VtraceIO(*[P] * len(N.VTRACE_IO_FIELDS))
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _call(d, io):
    lib = N.load()
    rc = lib.aaa_vtrace(ctypes.byref(d) if d is not None else None, ctypes.byref(io) if io is not None else None, None)
    return rc, lib.aaa_last_error()


def test_symbol_is_exported_and_bound():
    assert "aaa_vtrace" in N.EXPORTS
    assert hasattr(N.load(), "aaa_vtrace")
    assert [n for n, _ in N.VtraceIO._fields_] == list(REQUIRED[:4] + OPTIONAL[:3] + REQUIRED[4:] + OPTIONAL[3:])
    assert ctypes.sizeof(N.VtraceDesc) == 4 * 4 + 8 * 8 and ctypes.sizeof(N.VtraceIO) == 12 * 8


def test_refuses_null_desc_and_io():
    for d, io in ((None, _io()), (_desc(), None), (None, None)):
        rc, msg = _call(d, io)
        assert rc == -1 and b"NULL" in msg


@pytest.mark.parametrize("field", REQUIRED)
def test_refuses_null_required_pointer(field):
    rc, msg = _call(_desc(), _io(**{field: None}))
    assert rc == -1 and b"NULL" in msg


BAD_DESC = {
    "T = 0": dict(T=0), "B = 0": dict(B=0), "A = 1": dict(A=1), "T < 0": dict(T=-3),
    "value_col = -1": dict(value_col=-1), "value_col = A": dict(value_col=18),
    "gamma > 1": dict(gamma=1.5), "gamma < 0": dict(gamma=-0.1), "gamma nan": dict(gamma=math.nan),
    "lambda > 1": dict(lam=1.01), "lambda < 0": dict(lam=-1.0), "lambda nan": dict(lam=math.nan),
    "rho_bar = 0": dict(rho_bar=0.0), "rho_bar inf": dict(rho_bar=math.inf), "rho_bar nan": dict(rho_bar=math.nan),
    "c_bar < 0": dict(c_bar=-1.0), "c_bar inf": dict(c_bar=math.inf),
    "pg_rho_bar = 0": dict(pg_rho_bar=0.0), "pg_rho_bar nan": dict(pg_rho_bar=math.nan),
    "baseline_cost < 0": dict(baseline_cost=-0.5), "baseline_cost inf": dict(baseline_cost=math.inf),
    "entropy_cost < 0": dict(entropy_cost=-0.01), "entropy_cost nan": dict(entropy_cost=math.nan),
    "scale < 0": dict(scale=-1.0), "scale inf": dict(scale=math.inf), "scale nan": dict(scale=math.nan),
}


@pytest.mark.parametrize("what", sorted(BAD_DESC))
def test_refuses_bad_desc(what):
    rc, msg = _call(_desc(**BAD_DESC[what]), _io())
    assert rc == -1 and msg.startswith(b"vtrace"), (what, rc, msg)


@pytest.mark.parametrize("field", ["dlogits", "dvalues"])
def test_refuses_misaligned_cotangent_buffers(field):
    for off in (4, 8, 12):
        rc, msg = _call(_desc(), _io(**{field: P + off}))
        assert rc == -2 and b"aligned" in msg, (field, off)   # AAA_E_ALIGN


def test_argument_errors_come_first_with_optional_pointers_null():
    """The optional pointers may be NULL: with them NULL a bad desc is still
    what is refused (AAA_E_ARG), not the NULLs."""
    rc, msg = _call(_desc(A=1), _io(**{k: None for k in OPTIONAL}))
    assert rc == -1 and b"A >= 2" in msg


def test_vtrace_loss_has_no_cpu_fallback():
    import torch
    from aaa_amd.vtrace import vtrace_loss
    z = torch.zeros(3, 1, 18)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vtrace_loss(z, z, [0, 1, 2], [1.0, 0.0, 1.0])
