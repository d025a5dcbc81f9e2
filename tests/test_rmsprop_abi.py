"""CPU-side checks of the RMSProp entry (include/aaa.h aaa_rmsprop_step): the
symbol is exported and bound without an ABI bump, and every argument it refuses
is refused with the stated code and an "rmsprop" message before any device call
(no GPU needed; the addresses are dummies, and only refused calls are sent)."""
import ctypes
import inspect
import math

import pytest

from helpers import ROOT, detinit  # noqa: F401  (path setup)

import attention  # noqa: F401
from aaa_amd import _native as N

P = 4096        # a dummy aligned address, never dereferenced: every call here is refused before the device
E_ARG, E_ALIGN = -1, -2
ARRAYS = ("params", "grads", "square_avg", "momentum_buf", "grad_avg")


def _arr(*ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _numel(*n):
    return (ctypes.c_size_t * max(len(n), 1))(*n)


def _hp(**kw):
    f = dict(lr=1e-3, alpha=0.99, eps=0.01, weight_decay=0.0, momentum=0.0, lr_end=0.0, anneal_steps=0, centered=0,
             maximize=0, eps_in_sqrt=1)
    f.update(kw)
    return N.RmspropHP(f["lr"], f["alpha"], f["eps"], f["weight_decay"], f["momentum"], f["lr_end"], f["anneal_steps"],
                       f["centered"], f["maximize"], f["eps_in_sqrt"])


def _call(hp="ok", step=1, step_dev=P, guard=P, stats=P, n=2, arrays=None, numel="ok", **hpkw):
    a = {k: _arr(P, P + 64) for k in ARRAYS}
    a.update(arrays or {})
    numel = _numel(5, 7) if numel == "ok" else numel
    hp = ctypes.byref(_hp(**hpkw)) if hp == "ok" else hp
    return N.load().aaa_rmsprop_step(hp, step, step_dev, guard, stats, n, a["params"], a["grads"], a["square_avg"],
                                     a["momentum_buf"], a["grad_avg"], numel, None)


def _refused(rc, code, word=None):
    msg = N.load().aaa_last_error()
    assert rc == code and msg.startswith(b"rmsprop"), (rc, msg)
    if word:
        assert word in msg, msg


def test_symbol_is_exported_and_bound():
    lib = N.load()
    assert "aaa_rmsprop_step" in N.EXPORTS and hasattr(lib, "aaa_rmsprop_step")
    assert lib.aaa_rmsprop_step.argtypes is not None and len(lib.aaa_rmsprop_step.argtypes) == 13
    assert lib.aaa_abi_version() == N.ABI_VERSION == 12   # additive: no ABI bump
    assert callable(N.rmsprop_step)
    # the struct as include/aaa.h lays it out: 6 doubles, a long, 3 ints (+ tail padding)
    assert [f[0] for f in N.RmspropHP._fields_] == ["lr", "alpha", "eps", "weight_decay", "momentum", "lr_end",
                                                    "anneal_steps", "centered", "maximize", "eps_in_sqrt"]
    assert ctypes.sizeof(N.RmspropHP) == 6 * 8 + ctypes.sizeof(ctypes.c_long) + 16
    assert N.RmspropHP.anneal_steps.offset == 48 and N.RmspropHP.centered.offset == 48 + ctypes.sizeof(ctypes.c_long)


def test_refuses_null_hp_and_arrays():
    _refused(_call(hp=None), E_ARG, b"NULL")
    for k in ("params", "grads", "square_avg"):
        _refused(_call(arrays={k: None}), E_ARG, b"NULL")
    _refused(_call(numel=None), E_ARG, b"NULL")
    # an array the variant needs
    _refused(_call(arrays={"momentum_buf": None}, momentum=0.9), E_ARG, b"momentum_buf")
    _refused(_call(arrays={"grad_avg": None}, centered=1), E_ARG, b"grad_avg")
    _refused(_call(arrays={"momentum_buf": None, "grad_avg": None}, momentum=0.5, centered=1), E_ARG, b"NULL")


def test_refuses_null_tensor_pointers():
    for k in ("params", "grads", "square_avg"):
        _refused(_call(arrays={k: _arr(P, None)}), E_ARG, b"tensor 1")
        _refused(_call(arrays={k: _arr(None, P)}), E_ARG, b"tensor 0")
    _refused(_call(arrays={"momentum_buf": _arr(P, None)}, momentum=0.9), E_ARG, b"tensor 1")
    _refused(_call(arrays={"grad_avg": _arr(None, P)}, centered=1), E_ARG, b"tensor 0")
    # (a NULL pointer of an EMPTY tensor, or in an array the variant does not use, is allowed -- so it is no
    # refusal and is not sent from here: tests/test_gpu_rmsprop.py runs both on real memory)


def test_refuses_negative_ntensors():
    _refused(_call(n=-1), E_ARG, b"ntensors")
    _refused(_call(n=-48), E_ARG, b"ntensors")


@pytest.mark.parametrize("field", ["lr", "lr_end", "alpha", "eps", "weight_decay", "momentum"])
@pytest.mark.parametrize("value", [-1e-9, -1.0, -math.inf, math.nan])
def test_refuses_negative_or_nan_hyper_parameters(field, value):
    _refused(_call(**{field: value}), E_ARG, b"hyper-parameters")


def test_refuses_negative_anneal_steps():
    _refused(_call(anneal_steps=-1), E_ARG, b"anneal_steps")


def test_refuses_step_below_one_without_a_device_counter():
    _refused(_call(step=0, step_dev=None), E_ARG, b"step")
    _refused(_call(step=-3, step_dev=None), E_ARG, b"step")


def test_refuses_misaligned_stats():
    for off in (4, 8, 12):
        _refused(_call(stats=P + off), E_ALIGN, b"aligned")
        _refused(_call(stats=P + off, step_dev=None, guard=None), E_ALIGN, b"aligned")


def test_python_surface_without_gpu():
    import torch
    from aaa_amd.optim import RMSprop, rmsprop_flat_
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RMSprop([p]).step()
    with pytest.raises(RuntimeError, match="differentiable"):
        RMSprop([p], differentiable=True)
    # torch's validation, word for word
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate: -1.0"), (dict(eps=-1.0), "Invalid epsilon value: -1.0"),
                    (dict(momentum=-1.0), "Invalid momentum value: -1.0"),
                    (dict(weight_decay=-1.0), "Invalid weight_decay value: -1.0"),
                    (dict(alpha=-1.0), "Invalid alpha value: -1.0")):
        with pytest.raises(ValueError, match=msg):
            RMSprop([p], **kw)
        with pytest.raises(ValueError, match=msg):
            torch.optim.RMSprop([p], **kw)
    with pytest.raises(ValueError, match="lr_end"):
        RMSprop([p], lr_end=-1.0)
    with pytest.raises(ValueError, match="anneal_steps"):
        RMSprop([p], anneal_steps=-1)
    # torch's constructor, positionally; the extensions keyword-only
    ours, theirs = inspect.signature(RMSprop.__init__).parameters, inspect.signature(torch.optim.RMSprop.__init__).parameters
    assert list(ours)[:len(theirs)] == list(theirs)
    for k in theirs:
        assert ours[k].default == theirs[k].default, k
    for k, d in (("eps_in_sqrt", False), ("lr_end", 0.0), ("anneal_steps", 0)):
        assert ours[k].kind is inspect.Parameter.KEYWORD_ONLY and ours[k].default == d
    flat = inspect.signature(rmsprop_flat_).parameters
    assert list(flat)[:4] == ["params", "grads", "square_avg", "step"]
    for k in ("momentum_buf", "grad_avg", "guard", "step_dev", "clip"):
        assert flat[k].kind is inspect.Parameter.KEYWORD_ONLY and flat[k].default is None


def test_learner_signature_and_refusals():
    from aaa_amd.learner import Learner
    sig = inspect.signature(Learner.__init__).parameters
    assert sig["optimizer"].default == "adam" and sig["lr_anneal_steps"].default == 0 and sig["lr_end"].default == 0.0
    assert Learner.RMSPROP_DEFAULTS == dict(alpha=0.99, eps=0.01, momentum=0.0, centered=False, eps_in_sqrt=True)
    assert callable(Learner.current_lr)
    # refused before anything is allocated (no GPU needed)
    with pytest.raises(ValueError, match="lr_anneal_steps"):
        Learner(B=2, T=3, lr_anneal_steps=10)
    with pytest.raises(ValueError, match="optimizer"):
        Learner(B=2, T=3, optimizer="sgd")
    with pytest.raises(ValueError, match="unknown rmsprop"):
        Learner(B=2, T=3, optimizer="rmsprop", rmsprop=dict(beta=0.9))
