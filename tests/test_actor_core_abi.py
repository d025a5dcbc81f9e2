"""CPU-side checks of the stateful-core actor entry (aaa_actor_step_core,
include/aaa.h): its workspace query accepts what the chain runs and returns 0
for what it refuses, and the step refuses those configurations and a NULL core
state with AAA_E_ARG before any device call (no GPU needed)."""
import ctypes

import pytest

from helpers import ROOT  # noqa: F401  (path setup)

import attention  # noqa: F401
from aaa_amd import _native as N

SC = N.FLAG_STATEFUL_CORE | N.FLAG_FRAMES_U8

ACCEPTED = [N.Cfg(1, 1, 84, 84, 4, 18, N.F32, SC), N.Cfg(16, 1, 84, 84, 4, 18, N.F32, SC),
            N.Cfg(1, 1, 210, 160, 8, 18, N.F32, SC)]
REFUSED = {
    "flag missing": N.Cfg(1, 1, 84, 84, 4, 18, N.F32, N.FLAG_FRAMES_U8),
    "bf16": N.Cfg(1, 1, 84, 84, 4, 18, N.BF16, SC),
    "T = 2": N.Cfg(1, 2, 84, 84, 4, 18, N.F32, SC),
    "B = 17": N.Cfg(17, 1, 84, 84, 4, 18, N.F32, SC),
    "506x506": N.Cfg(1, 1, 506, 506, 4, 18, N.F32, SC),
}


def test_core_workspace_query_accepts_supported():
    lib = N.load()
    sizes = [lib.aaa_actor_core_workspace_bytes(ctypes.byref(c)) for c in ACCEPTED]
    assert all(s > 0 for s in sizes), sizes
    # the query MLP's rows come on top of the zero-state chain's workspace
    plain = N.Cfg(1, 1, 84, 84, 4, 18, N.F32, N.FLAG_FRAMES_U8)
    assert sizes[0] > lib.aaa_actor_workspace_bytes(ctypes.byref(plain)) > 0


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_core_entry_refuses_unsupported(what):
    lib = N.load()
    cfg = REFUSED[what]
    assert lib.aaa_actor_core_workspace_bytes(ctypes.byref(cfg)) == 0, what
    io, core = N.ActorIO(), N.ActorCoreIO()
    assert lib.aaa_actor_step_core(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(core), None) == -1, what
    assert lib.aaa_last_error()


def test_core_entry_refuses_null_core_state():
    """NULL ``core``, and a core without core_h / core_c, with every aaa_actor_io
    pointer set (to a dummy aligned address that is never dereferenced: the
    refusal comes before the device is touched)."""
    lib = N.load()
    cfg = ACCEPTED[0]
    io = N.ActorIO()
    for name in ("params", "packed", "basis", "frames", "h", "c", "logits", "values", "workspace"):
        setattr(io, name, 4096)
    assert lib.aaa_actor_step_core(ctypes.byref(cfg), ctypes.byref(io), None, None) == -1
    assert b"core" in lib.aaa_last_error()
    core = N.ActorCoreIO()
    assert lib.aaa_actor_step_core(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(core), None) == -1
    core.core_h = 4096
    assert lib.aaa_actor_step_core(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(core), None) == -1
    assert b"core" in lib.aaa_last_error()
    # and with an empty io as well
    assert lib.aaa_actor_step_core(ctypes.byref(cfg), ctypes.byref(N.ActorIO()), None, None) == -1


def test_zero_state_entry_still_refuses_the_flag():
    lib = N.load()
    cfg = ACCEPTED[0]
    assert lib.aaa_actor_workspace_bytes(ctypes.byref(cfg)) == 0
    assert lib.aaa_actor_step(ctypes.byref(cfg), ctypes.byref(N.ActorIO()), None) == -1


def test_graph_actor_fit_query_knows_the_mode():
    from aaa_amd.policy import _actor_chain_fits
    assert _actor_chain_fits(2, 84, 84, 4, 18, True) and _actor_chain_fits(2, 84, 84, 4, 18)
    assert not _actor_chain_fits(1, 506, 506, 4, 18, True) and not _actor_chain_fits(17, 84, 84, 4, 18, True)
