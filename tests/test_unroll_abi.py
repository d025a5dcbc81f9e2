"""CPU-side checks of the unroll recorder's entries (include/aaa.h
aaa_unroll_begin / aaa_unroll_record): the symbols are exported and bound
without an ABI bump, the structs are laid out as the header states, and every
argument they refuse is refused with the stated code and an "unroll" message
before any device call (no GPU needed; the addresses are dummies, and only
refused calls are sent)."""
import ctypes
import inspect
import math

import pytest

from helpers import ROOT, detinit  # noqa: F401  (path setup)

import attention  # noqa: F401
from aaa_amd import _native as N

P = 1 << 20     # a dummy aligned address, never dereferenced: every call here is refused before the device
E_ARG, E_ALIGN = -1, -2
BANK_STATE = ("h0", "c0", "core_h0", "core_c0")
LIVE_STATE = ("h", "c", "core_h", "core_c")
BEGIN_NEEDS = dict(io=("pos", "done_in", "h", "c"), bank=("first", "h0", "c0"))
RECORD_NEEDS = dict(io=("pos", "frame", "actions", "logp", "reward_in", "done_in"),
                    bank=("frames", "actions", "logp", "rewards", "done"))


def _desc(**kw):
    f = dict(T=3, B=3, Bu=5, b0=1, frame_bytes=48, state_floats=8, core=256, reward_clip=0.0)
    f.update(kw)
    return N.UnrollDesc(f["T"], f["B"], f["Bu"], f["b0"], f["frame_bytes"], f["state_floats"], f["core"],
                        f["reward_clip"])


def _io(io=None, bank0=None, bank1=None):
    """Every pointer a distinct 4096-aligned dummy; the dicts override fields (None: NULL)."""
    x = N.UnrollIO()
    addr = P
    for k in (0, 1):
        for name in N.UNROLL_BANK_FIELDS:
            setattr(x.bank[k], name, addr)
            addr += 4096
    for name in N.UNROLL_IO_FIELDS:
        setattr(x, name, addr)
        addr += 4096
    for k, over in ((0, bank0), (1, bank1)):
        for name, v in (over or {}).items():
            setattr(x.bank[k], name, v)
    for name, v in (io or {}).items():
        setattr(x, name, v)
    return x


def _call(which, desc="ok", io="ok", **kw):
    fn = getattr(N.load(), "aaa_unroll_" + which)
    d = ctypes.byref(_desc(**kw)) if desc == "ok" else desc
    i = ctypes.byref(_io() if io == "ok" else io) if io is not None else None
    return fn(d, i, None)


def _refused(rc, code, word=None):
    msg = N.load().aaa_last_error()
    assert rc == code and msg.startswith(b"unroll"), (rc, msg)
    if word:
        assert word in msg, msg


BOTH = pytest.mark.parametrize("which", ["begin", "record"])


def test_symbols_are_exported_and_bound():
    lib = N.load()
    for name in ("aaa_unroll_begin", "aaa_unroll_record"):
        assert name in N.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 3
    assert lib.aaa_abi_version() == N.ABI_VERSION == 12   # additive: no ABI bump
    assert callable(N.unroll_begin) and callable(N.unroll_record)


def test_struct_layout_is_the_header():
    assert [f[0] for f in N.UnrollDesc._fields_] == ["T", "B", "Bu", "b0", "frame_bytes", "state_floats", "core",
                                                     "reward_clip"]
    assert (N.UnrollDesc.frame_bytes.offset, N.UnrollDesc.state_floats.offset, N.UnrollDesc.core.offset,
            N.UnrollDesc.reward_clip.offset, ctypes.sizeof(N.UnrollDesc)) == (16, 24, 32, 40, 48)
    assert [f[0] for f in N.UnrollBank._fields_] == ["frames", "actions", "logp", "rewards", "done", "first", "h0",
                                                     "c0", "core_h0", "core_c0"]
    assert ctypes.sizeof(N.UnrollBank) == 80
    assert [f[0] for f in N.UnrollIO._fields_] == ["bank", "pos", "frame", "actions", "logp", "reward_in", "done_in",
                                                   "h", "c", "core_h", "core_c"]
    assert N.UnrollIO.pos.offset == 160 and ctypes.sizeof(N.UnrollIO) == 240
    # the header declares them in this order
    src = open(ROOT + "/include/aaa.h").read()
    body = src[src.index("typedef struct aaa_unroll_desc"):src.index("int aaa_unroll_begin")]
    names = [n for n in ("T;", "B;", "Bu, b0;", "frame_bytes;", "state_floats;", "core;", "reward_clip;", "frames;",
                         "actions;", "*logp, *rewards, *done;", "first;", "*h0, *c0;", "*core_h0, *core_c0;",
                         "bank[2];", "pos;", "frame;", "actions;", "logp;", "*reward_in, *done_in;",
                         "*h, *c, *core_h, *core_c;")]
    at = 0
    for n in names:
        at = body.index(n, at) + 1


@BOTH
def test_refuses_null_desc_or_io(which):
    _refused(_call(which, desc=None), E_ARG, b"NULL")
    _refused(_call(which, io=None), E_ARG, b"NULL")


@BOTH
@pytest.mark.parametrize("kw,word", [
    (dict(T=1), b"T must"), (dict(T=0), b"T must"), (dict(T=-3), b"T must"),
    (dict(B=0), b"B must"), (dict(B=-1), b"B must"),
    (dict(b0=-1), b"rows"), (dict(b0=3), b"rows"), (dict(B=6, b0=0), b"rows"), (dict(Bu=3), b"rows"),
    (dict(frame_bytes=0), b"frame_bytes"),
    (dict(state_floats=6), b"state_floats"), (dict(state_floats=1), b"state_floats"), (dict(state_floats=7), b"state_floats"),
    (dict(core=1), b"core"), (dict(core=128), b"core"), (dict(core=-256), b"core"), (dict(core=512), b"core"),
    (dict(reward_clip=-1e-9), b"reward_clip"), (dict(reward_clip=-1.0), b"reward_clip"),
    (dict(reward_clip=-math.inf), b"reward_clip"), (dict(reward_clip=math.nan), b"reward_clip"),
])
def test_refuses_bad_desc(which, kw, word):
    _refused(_call(which, **kw), E_ARG, word)


@pytest.mark.parametrize("which,needs", [("begin", BEGIN_NEEDS), ("record", RECORD_NEEDS)])
def test_refuses_null_required_pointers(which, needs):
    for name in needs["io"]:
        _refused(_call(which, io=_io(io={name: None})), E_ARG, b"NULL")
    for k in (0, 1):
        for name in needs["bank"]:
            _refused(_call(which, io=_io(**{f"bank{k}": {name: None}})), E_ARG, b"NULL")


def test_refuses_null_core_pointers_with_core_256():
    for name in ("core_h", "core_c"):
        _refused(_call("begin", io=_io(io={name: None})), E_ARG, b"core")
    for k in (0, 1):
        for name in ("core_h0", "core_c0"):
            _refused(_call("begin", io=_io(**{f"bank{k}": {name: None}})), E_ARG, b"core")
    # (with core = 0 they may be NULL and are never read: no refusal, so nothing is sent from here;
    # tests/test_gpu_unroll.py runs that on real memory)


@BOTH
def test_refuses_misaligned_pos_and_state(which):
    for off in (4, 8, 12):
        _refused(_call(which, io=_io(io={"pos": P + off})), E_ALIGN, b"aligned")
        for name in LIVE_STATE:
            _refused(_call(which, io=_io(io={name: P + off})), E_ALIGN, b"aligned")
        for k in (0, 1):
            for name in BANK_STATE:
                _refused(_call(which, io=_io(**{f"bank{k}": {name: P + off}})), E_ALIGN, b"aligned")


@BOTH
def test_refuses_misaligned_frames_only_when_rows_are_16_byte_multiples(which):
    for fb in (48, 4800, 84 * 84 * 3, 210 * 160 * 3):
        assert fb % 16 == 0
        for off in (1, 4, 8):
            _refused(_call(which, io=_io(io={"frame": P + off}), frame_bytes=fb), E_ALIGN, b"frame")
            for k in (0, 1):
                _refused(_call(which, io=_io(**{f"bank{k}": {"frames": P + off}}), frame_bytes=fb), E_ALIGN, b"frame")


def test_python_surface_without_gpu():
    from aaa_amd.learner import Learner
    from aaa_amd.policy import GraphActor
    from aaa_amd.unroll import Unroll, UnrollCollector, completed_unrolls
    assert Unroll._fields == ("frames", "actions", "rewards", "logp", "done", "first", "initial_state")
    assert [completed_unrolls(n, 3) for n in range(8)] == [0, 0, 0, 1, 1, 2, 2, 3]
    sig = inspect.signature(UnrollCollector.__init__).parameters
    assert list(sig)[1:5] == ["T", "B", "H", "W"]
    assert sig["stateful_core"].default is False and sig["reward_clip"].default == 0.0
    assert inspect.signature(UnrollCollector.take).parameters["copy"].default is False
    for name in ("rows", "ready", "take", "restart"):
        assert callable(getattr(UnrollCollector, name))
    with pytest.raises(ValueError, match="T must be >= 2"):
        UnrollCollector(1, 2, 84, 84)
    with pytest.raises(ValueError, match="reward_clip"):
        UnrollCollector(3, 2, 84, 84, reward_clip=-1.0)
    assert inspect.signature(GraphActor.__init__).parameters["recorder"].default is None
    step = inspect.signature(GraphActor.step).parameters
    assert list(step) == ["self", "observation", "reward", "done"] and step["reward"].default is None
    for name in ("step", "step_vtrace", "train_step", "train_step_vtrace"):
        assert inspect.signature(getattr(Learner, name)).parameters["initial_state"].default is None, name
    assert inspect.signature(Learner.__init__).parameters["stateful_core"].default is False
    assert callable(Learner.train_on)
