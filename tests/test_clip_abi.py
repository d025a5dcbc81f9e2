"""CPU-side checks of the gradient-clipping entries (include/aaa.h
aaa_grad_norm_scratch_bytes / aaa_grad_norm / aaa_grad_scale /
aaa_adam_step_clipped): the symbols are exported and bound, the scratch size
is 8 bytes per 4096-element chunk, and every argument they refuse is refused
with the stated code and a "clip" message before any device call (no GPU
needed; the addresses are dummies)."""
import ctypes
import math

import numpy as np
import pytest

from helpers import ROOT, detinit  # noqa: F401  (path setup)

import attention  # noqa: F401
from aaa_amd import _native as N

P = 4096        # a dummy aligned address, never dereferenced: only refused calls are sent, and every
                # refusal comes before the device
CHUNK = 4096    # csrc/optim.hip kAdamChunk
NAMES = ("aaa_grad_norm_scratch_bytes", "aaa_grad_norm", "aaa_grad_scale", "aaa_adam_step_clipped")
E_ARG, E_ALIGN = -1, -2


def _arr(*ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _numel(*n):
    return (ctypes.c_size_t * max(len(n), 1))(*n)


def _hp():
    return N.AdamHP(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)


def _refused(rc, code, word=None):
    msg = N.load().aaa_last_error()
    assert rc == code and msg.startswith(b"clip"), (rc, msg)
    if word:
        assert word in msg, msg


def test_symbols_are_exported_and_bound():
    lib = N.load()
    for name in NAMES:
        assert name in N.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.aaa_grad_norm_scratch_bytes.restype is ctypes.c_size_t
    assert lib.aaa_abi_version() == 12   # additive: no ABI bump
    assert callable(N.grad_norm) and callable(N.grad_scale) and callable(N.grad_norm_scratch_bytes)


def test_scratch_bytes():
    def expect(numels):
        chunks = sum(-(-n // CHUNK) for n in numels)
        return max(16, (8 * chunks + 15) // 16 * 16)
    ref = [int(np.prod(s)) for _, s in detinit.param_shapes(18, 4)]
    assert len(ref) == 34
    for numels, want in (([], 16), ([0], 16), ([1], 16), ([CHUNK], 16), ([CHUNK + 1], 16), ([2 * CHUNK + 1], 32),
                         ([CHUNK + 1, 1], 32), (ref, None), ([sum(ref)], 8 * 555 + 8)):
        got = N.grad_norm_scratch_bytes(numels)
        assert got == expect(numels) and got % 16 == 0 and got >= 16, (numels, got)
        if want is not None:
            assert got == want, (numels, got, want)
    assert N.load().aaa_grad_norm_scratch_bytes(0, None) == 16


def _grad_norm(max_norm=1.0, n=2, grads="ok", numel="ok", stats=P, scratch=P):
    grads = _arr(P, P + 64) if grads == "ok" else grads
    numel = _numel(5, 7) if numel == "ok" else numel
    return N.load().aaa_grad_norm(max_norm, n, grads, numel, stats, scratch, None)


def test_grad_norm_refuses_null_and_negative():
    _refused(_grad_norm(grads=None), E_ARG, b"NULL")
    _refused(_grad_norm(numel=None), E_ARG, b"NULL")
    _refused(_grad_norm(stats=None), E_ARG, b"NULL")
    _refused(_grad_norm(scratch=None), E_ARG, b"NULL")
    _refused(_grad_norm(grads=_arr(P, None)), E_ARG, b"tensor 1")
    _refused(_grad_norm(n=-1), E_ARG, b"ntensors")


@pytest.mark.parametrize("max_norm", [0.0, -1.0, -math.inf, math.nan])
def test_grad_norm_refuses_bad_max_norm(max_norm):
    _refused(_grad_norm(max_norm=max_norm), E_ARG, b"max_norm")


@pytest.mark.parametrize("which", ["stats", "scratch"])
def test_grad_norm_refuses_misaligned(which):
    for off in (4, 8, 12):
        _refused(_grad_norm(**{which: P + off}), E_ALIGN, b"aligned")


def test_grad_scale_refusals():
    lib = N.load()
    ok_g, ok_n = _arr(P, P + 64), _numel(5, 7)
    _refused(lib.aaa_grad_scale(None, 2, ok_g, ok_n, None), E_ARG, b"NULL")
    _refused(lib.aaa_grad_scale(P, 2, None, ok_n, None), E_ARG, b"NULL")
    _refused(lib.aaa_grad_scale(P, 2, ok_g, None, None), E_ARG, b"NULL")
    _refused(lib.aaa_grad_scale(P, 2, _arr(None, P), ok_n, None), E_ARG, b"tensor 0")
    _refused(lib.aaa_grad_scale(P, -2, ok_g, ok_n, None), E_ARG, b"ntensors")
    _refused(lib.aaa_grad_scale(P + 8, 2, ok_g, ok_n, None), E_ALIGN, b"aligned")


def _clipped(step_dev=P, guard=P, stats=P, n=2, arrays=None, numel="ok", hp="ok"):
    a = {k: _arr(P, P + 64) for k in ("params", "grads", "exp_avg", "exp_avg_sq")}
    a.update(arrays or {})
    numel = _numel(5, 7) if numel == "ok" else numel
    hp = ctypes.byref(_hp()) if hp == "ok" else hp
    return N.load().aaa_adam_step_clipped(hp, step_dev, guard, stats, n, a["params"], a["grads"], a["exp_avg"],
                                          a["exp_avg_sq"], None, numel, None)


def test_adam_step_clipped_refusals():
    _refused(_clipped(step_dev=None), E_ARG, b"NULL")
    _refused(_clipped(stats=None), E_ARG, b"NULL")
    _refused(_clipped(stats=P + 4), E_ALIGN, b"aligned")
    _refused(_clipped(n=-1), E_ARG)
    _refused(_clipped(hp=None), E_ARG, b"NULL")
    _refused(_clipped(numel=None), E_ARG, b"NULL")
    for k in ("params", "grads", "exp_avg", "exp_avg_sq"):
        _refused(_clipped(arrays={k: None}), E_ARG, b"NULL")
        _refused(_clipped(arrays={k: _arr(P, None)}), E_ARG, b"tensor 1")
    # guard = NULL is allowed, so it is no refusal: tests/test_gpu_clip.py runs it on real memory
    # (a well-formed call would reach the device wherever one is visible, so none is sent from here)


def test_python_surface_without_gpu():
    import torch
    from aaa_amd.optim import clip_grad_norm_
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clip_grad_norm_([p], 1.0)
    with pytest.raises(ValueError, match="norm_type"):
        clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(ValueError, match="step_dev"):
        N.adam_step(_hp(), 1, [], [], [], [], clip=torch.zeros(4))
    # torch's signature, positionally
    import inspect
    names = list(inspect.signature(clip_grad_norm_).parameters)
    assert names[:5] == ["parameters", "max_norm", "norm_type", "error_if_nonfinite", "foreach"]


def test_learner_signature_has_max_grad_norm():
    import inspect
    from aaa_amd.learner import Learner
    assert inspect.signature(Learner.__init__).parameters["max_grad_norm"].default is None
    assert callable(Learner.clip_report)
