"""CPU-side checks of the C ABI: the library loads, exports every symbol
include/aaa.h declares, and its layout queries agree with the reference's
state_dict (no GPU compute is issued here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import ROOT, detinit

import attention  # noqa: F401
from aaa_amd import _native as N

HEADER = os.path.join(ROOT, "include", "aaa.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(aaa_[a-z0-9_]+)\s*\(", src)))


def test_header_matches_binding_list():
    assert _declared() == sorted(N.EXPORTS)


def test_library_exports_every_declared_symbol():
    lib = N.load()
    for name in _declared():
        assert hasattr(lib, name), name


def test_abi_version():
    assert N.load().aaa_abi_version() == N.ABI_VERSION == 12


def test_core_checker_regions():
    """ABI 11: the fp32 recurrence's operand slots, the readout's cotangent of
    h_t and the cotangent of conv2's output as workspace regions -- their sizes,
    that they lie inside the workspace without overlapping, and AAA_E_ARG for a
    bf16 config (as aaa_core_export refuses what it cannot give as fp32 rows)."""
    lib = N.load()
    src = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"AAA_WS_([A-Z0-9_]+)\s*=\s*(\d+)", src))
    core = {"ANSWER_HIDDEN": 0, "QUERY_HIDDEN0": 1, "QUERY_HIDDEN1": 2, "CORE_XH": 3, "CORE_DO": 4, "CORE_DX": 5}
    assert {k: v for k, v in enum.items() if not k.startswith("TAIL_")} == core
    assert sorted(enum.values()) == list(range(len(enum)))
    for name, val in enum.items():
        assert getattr(N, "WS_" + name) == val, name
    T, B, P = 20, 32, 121
    cfg = N.Cfg(B, T, 84, 84, 4, 18, N.F32, 0)
    ws = lib.aaa_workspace_bytes(ctypes.byref(cfg))
    spans = []
    for region, nbytes in ((N.WS_CORE_XH, (T + 1) * B * P * 192 * 4), (N.WS_CORE_DO, T * B * P * 128 * 4),
                           (N.WS_CORE_DX, T * B * P * 64 * 4)):
        off, nb = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.aaa_workspace_region(ctypes.byref(cfg), region, ctypes.byref(off), ctypes.byref(nb)) == 0
        assert nb.value == nbytes and off.value % 16 == 0 and off.value + nb.value <= ws
        spans.append((off.value, off.value + nb.value))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    bf = N.Cfg(B, T, 84, 84, 4, 18, N.BF16, 0)
    for region in (N.WS_CORE_XH, N.WS_CORE_DO, N.WS_CORE_DX):
        assert lib.aaa_workspace_region(ctypes.byref(bf), region, ctypes.byref(off), ctypes.byref(nb)) == -1
        assert b"region" in lib.aaa_last_error()
    assert lib.aaa_workspace_region(ctypes.byref(bf), N.WS_ANSWER_HIDDEN, ctypes.byref(off), ctypes.byref(nb)) == 0
    for unknown in (-1, len(enum)):
        assert lib.aaa_workspace_region(ctypes.byref(cfg), unknown, ctypes.byref(off), ctypes.byref(nb)) == -1


def test_tail_checker_regions():
    """ABI 12: the policy tail's operands, products and cotangents as workspace regions -- granted for fp32 and
    bf16 configs alike (fp32 buffers in both), their sizes from the cfg, inside the workspace, no two overlapping
    (nor the older regions), and AAA_E_ARG for the regions of the other core kind."""
    lib = N.load()
    T, B = 3, 9
    every = ("ANS", "GATES", "DY", "DGATES", "DHID", "DANS")
    zero = ("AO", "C", "H", "DAO")
    state = ("AOX", "CH", "CC", "QUERY", "DAOX", "DQUERY", "DQ2", "DQ1")
    assert sorted(every + zero + state) == sorted(k[8:] for k in dir(N) if k.startswith("WS_TAIL_"))
    for nq, A in ((4, 18), (8, 5)):
        F, qd, ans_ld, ldy = T * B, 72 * nq, (256 * nq + 2 + 7) // 8 * 8, (2 * A + 3) // 4 * 4
        for dt in (N.F32, N.BF16):
            for sc in (0, 1):
                cfg = N.Cfg(B, T, 84, 84, nq, A, dt, N.FLAG_STATEFUL_CORE if sc else 0)
                ws = lib.aaa_workspace_bytes(ctypes.byref(cfg))
                cols = {"ANS": ans_ld, "GATES": 1024, "DY": ldy, "DGATES": 1024, "DHID": 512,
                        "DANS": (256 if sc else 184) * nq, "AO": 256, "C": 256, "H": 256, "DAO": 256, "AOX": 512,
                        "DAOX": 512, "QUERY": qd, "DQUERY": qd, "DQ2": qd, "DQ1": 128}
                spans = []
                off, nb = ctypes.c_size_t(), ctypes.c_size_t()
                for name in every + (state if sc else zero) + ("ANSWER_HIDDEN",) + (("QUERY_HIDDEN0", "QUERY_HIDDEN1") if sc else ()):
                    rc = lib.aaa_workspace_region(ctypes.byref(cfg), getattr(N, "WS_" + ("" if "HIDDEN" in name else "TAIL_") + name),
                                                  ctypes.byref(off), ctypes.byref(nb))
                    assert rc == 0, (name, nq, dt, sc)
                    if "HIDDEN" not in name:
                        want = (T + 1) * B * 256 * 4 if name in ("CH", "CC") else F * cols[name] * 4
                        assert nb.value == want, (name, nb.value, want)
                    assert off.value % 16 == 0 and off.value + nb.value <= ws, name
                    spans.append((off.value, off.value + nb.value, name))
                spans.sort()
                assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
                for name in (zero if sc else state):
                    assert lib.aaa_workspace_region(ctypes.byref(cfg), getattr(N, "WS_TAIL_" + name), ctypes.byref(off),
                                                    ctypes.byref(nb)) == -1, name
                    assert b"region" in lib.aaa_last_error()


def test_bf16_core_checker_regions(monkeypatch):
    """After ABI 12, additive: the bf16 recurrence's buffers as workspace regions (AAA_BF16_WS_*) and
    aaa_core_layout -- granted for bf16 configs in every geometry (row-major per-step, channel-quad-major
    frame-resident and band mode), refused for fp32 ones; their sizes from the cfg and the gate storage type;
    inside the workspace, 16-byte aligned, no two overlapping (nor the tail's and the mask regions); and
    aaa_core_layout's mask is 0 exactly where aaa_core_elem_bytes reports non-zero sizes."""
    lib = N.load()
    src = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"AAA_BF16_WS_([A-Z0-9_]+)\s*=\s*(\d+)", src))
    assert enum == {"XH": 24, "C": 25, "GATES": 26, "DO": 27, "DZ": 28, "DX": 29}
    for name, val in enum.items():
        assert getattr(N, "BF16_WS_" + name) == val, name
    assert (N.CQM_C, N.CQM_G, N.CQM_DO) == (1, 2, 4)
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    ge, he, gl, mask = (ctypes.c_int() for _ in range(4))
    masks = set()
    # (env, B, T, H, W): per-step default, forced frame-resident / paired, the production batch, band mode and
    # the per-step launches on its grid, a grid neither kernel family takes
    geos = (({}, 2, 3, 84, 84), ({"AAA_FRAMES_FWD": "1", "AAA_FRAMES_BWD": "1"}, 2, 3, 84, 84),
            ({"AAA_FRAMES_FWD": "2", "AAA_FRAMES_BWD": "2"}, 9, 2, 84, 84),
            ({"AAA_FRAMES_FWD": "1", "AAA_FRAMES_BWD": "0"}, 3, 4, 64, 64), ({}, 256, 20, 84, 84),
            ({}, 5, 3, 168, 168), ({"AAA_FRAMES_BAND": "0"}, 5, 3, 168, 168), ({}, 1, 1, 210, 160))
    for env, B, T, H, W in geos:
        for k in ("AAA_FRAMES_FWD", "AAA_FRAMES_BWD", "AAA_FRAMES_BAND"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        h, w = N.grid(H, W)
        M = B * h * w
        cfg = N.Cfg(B, T, H, W, 4, 18, N.BF16, 0)
        ws = lib.aaa_workspace_bytes(ctypes.byref(cfg))
        assert lib.aaa_core_layout(ctypes.byref(cfg), ctypes.byref(gl), ctypes.byref(mask)) == 0
        assert lib.aaa_core_elem_bytes(ctypes.byref(cfg), ctypes.byref(ge), ctypes.byref(he)) == 0
        assert gl.value in (2, 4) and 0 <= mask.value <= 7
        assert (mask.value == 0) == (ge.value != 0) == (he.value != 0), (env, B, H, mask.value, ge.value)
        if ge.value:
            assert ge.value == gl.value and he.value == 2
        masks.add(mask.value)
        want = {"XH": (T + 1) * M * 192 * 2, "C": (T + 1) * M * 128 * 4, "GATES": T * M * 512 * gl.value,
                "DO": T * M * 128 * 4, "DZ": T * M * 512 * 2, "DX": T * M * 64 * 2}
        spans = []
        for name in list(want) + ["WS_ANSWER_HIDDEN", "WS_TAIL_ANS", "WS_TAIL_GATES", "WS_TAIL_DY", "WS_TAIL_DANS"]:
            region = getattr(N, name if name.startswith("WS_") else "BF16_WS_" + name)
            assert lib.aaa_workspace_region(ctypes.byref(cfg), region, ctypes.byref(off), ctypes.byref(nb)) == 0, name
            if name in want:
                assert nb.value == want[name], (name, nb.value, want[name])
            assert off.value % 16 == 0 and off.value + nb.value <= ws, name
            spans.append((off.value, off.value + nb.value, name))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
        f32 = N.Cfg(B, T, H, W, 4, 18, N.F32, 0)
        for name in want:
            assert lib.aaa_workspace_region(ctypes.byref(f32), getattr(N, "BF16_WS_" + name), ctypes.byref(off),
                                            ctypes.byref(nb)) == -1, name
            assert b"region" in lib.aaa_last_error()
        assert lib.aaa_core_layout(ctypes.byref(f32), ctypes.byref(gl), ctypes.byref(mask)) == 0
        assert (gl.value, mask.value) == (4, 0)
        assert lib.aaa_workspace_region(ctypes.byref(cfg), 30, ctypes.byref(off), ctypes.byref(nb)) == -1
    assert masks == {0, 7}, masks   # both layouts were seen
    assert lib.aaa_core_layout(ctypes.byref(cfg), None, ctypes.byref(mask)) == -1
    bad = N.Cfg(2, 3, 84, 84, 5, 18, N.BF16, 0)
    assert lib.aaa_core_layout(ctypes.byref(bad), ctypes.byref(gl), ctypes.byref(mask)) == -1


@pytest.mark.parametrize("H,W,hw", [(84, 84, (11, 11)), (168, 168, (21, 21)), (210, 160, (27, 20))])
def test_grid(H, W, hw):
    assert N.grid(H, W) == hw


@pytest.mark.parametrize("nq,total", [(4, 2270276), (8, 3080836)])
def test_param_layout_matches_state_dict(nq, total):
    cfg = N.Cfg(2, 3, 84, 84, nq, 18, N.F32, 0)
    n, offs, sizes = N.param_layout(cfg)
    assert n == total
    shapes = detinit.param_shapes(18, nq)
    assert sizes == [int(np.prod(s)) for _, s in shapes]
    assert offs == list(np.cumsum([0] + sizes[:-1]))


def test_layout_sizes_and_errors():
    lib = N.load()
    ok = N.Cfg(32, 20, 84, 84, 4, 18, N.F32, 0)
    ws = lib.aaa_workspace_bytes(ctypes.byref(ok))
    pk = lib.aaa_packed_bytes(ctypes.byref(ok))
    assert ws > 32 * 20 * 121 * 128 * 4 and pk > 512 * 1728 * 4
    bf = N.Cfg(32, 20, 84, 84, 4, 18, N.BF16, 0)
    assert lib.aaa_packed_bytes(ctypes.byref(bf)) < pk
    bad = N.Cfg(32, 20, 84, 84, 5, 18, N.F32, 0)
    assert lib.aaa_workspace_bytes(ctypes.byref(bad)) == 0
    assert b"nq" in lib.aaa_last_error()
    bad_rc = lib.aaa_forward(ctypes.byref(bad), None, None)
    assert bad_rc == -1


def test_agent_refuses_cpu_tensors():
    import torch
    agent = attention.Agent(18, grid=(11, 11))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        agent(torch.zeros(1, 84, 84, 3))


def test_state_dict_keys_match_reference_order():
    agent = attention.Agent(18)
    keys = list(agent.state_dict().keys())
    assert keys == [n for n, _ in detinit.param_shapes(18, 4)]
    assert len(list(agent.buffers())) == 0


def test_adam_rejects_bad_args_without_gpu():
    lib = N.load()
    hp = N.AdamHP(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)
    assert lib.aaa_adam_step(ctypes.byref(hp), 0, 0, None, None, None, None, None, None, None) == -1   # step < 1
    assert b"step" in lib.aaa_last_error()
    bad = N.AdamHP(1e-3, 1.0, 0.999, 1e-8, 0.0, 0, 0)
    assert lib.aaa_adam_step(ctypes.byref(bad), 1, 0, None, None, None, None, None, None, None) == -1
    ams = N.AdamHP(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0)
    one = (ctypes.c_void_p * 1)(16)
    n = (ctypes.c_size_t * 1)(4)
    assert lib.aaa_adam_step(ctypes.byref(ams), 1, 1, one, one, one, one, None, n, None) == -1     # amsgrad w/o vmax


def test_adam_optimizer_has_no_cpu_fallback():
    import torch
    from aaa_amd.optim import Adam
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Adam([p]).step()


def test_reinforce_rejects_bad_args_without_gpu():
    lib = N.load()
    assert lib.aaa_reinforce(0, 1, 18, 16, 16, 16, 0.99, 16, 16, 16, None) == -1
    assert lib.aaa_reinforce(4, 1, 18, None, 16, 16, 0.99, 16, 16, 16, None) == -1
    assert lib.aaa_reinforce(4, 1, 18, 16, 16, 16, 1.5, 16, 16, 16, None) == -1
    assert b"gamma" in lib.aaa_last_error()


def test_reinforce_loss_has_no_cpu_fallback():
    import torch
    from aaa_amd.reinforce import reinforce_loss
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reinforce_loss(torch.zeros(3, 1, 18), [0, 1, 2], [1.0, 0.0, 1.0])


def test_actor_layout_refuses_readout_overflow():
    """The actor chain's readout merges at most kActMaxChunks position chunks
    per frame (csrc/actor.h; P <= 2048): a larger grid is refused by the layout
    query (GraphActor then takes the learner's T=1 forward) instead of failing
    at launch."""
    lib = N.load()
    small = N.Cfg(1, 1, 210, 160, 8, 18, N.F32, N.FLAG_FRAMES_U8)
    big = N.Cfg(1, 1, 506, 506, 8, 18, N.F32, N.FLAG_FRAMES_U8)   # 64x64 grid: 4096 x 8 logits
    assert N.grid(506, 506) == (64, 64)
    assert lib.aaa_actor_workspace_bytes(ctypes.byref(small)) > 0
    assert lib.aaa_actor_workspace_bytes(ctypes.byref(big)) == 0


def test_timer_classes_match_header():
    """Every timer class the header enumerates has its binding constant (the
    bench reads all of them to attribute the whole step)."""
    src = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"AAA_TIMER_([A-Z_]+)\s*=\s*(\d+)", src))
    assert enum.pop("N") == N.TIMER_N == 12
    for name, val in enum.items():
        assert getattr(N, "TIMER_" + name) == val, name


def test_timing_stats_rejects_unknown_class():
    lib = N.load()
    s = N.TimerStats()
    assert lib.aaa_timing_stats(N.TIMER_N, ctypes.byref(s)) == -1
    assert lib.aaa_timing_stats(N.TIMER_MISC, ctypes.byref(s)) == 0 and s.launches == 0


def test_no_test_hooks_in_the_product_library():
    """The partner-wait budget has no override in libaaa.so:
    the stranded-launch tests strand a launch with a filler held past the
    default budget instead."""
    lib = N.load()
    assert not hasattr(lib, "aaa_debug_pair_spin")


def test_defer_stranded_flag_accepted():
    """AAA_FLAG_DEFER_STRANDED is a known cfg flag (layout queries need no GPU)."""
    lib = N.load()
    cfg = N.Cfg(2, 3, 84, 84, 4, 18, N.F32, N.FLAG_DEFER_STRANDED | N.FLAG_FRAMES_U8)
    assert lib.aaa_workspace_bytes(ctypes.byref(cfg)) > 0
    bad = N.Cfg(2, 3, 84, 84, 4, 18, N.F32, 8)
    assert lib.aaa_workspace_bytes(ctypes.byref(bad)) == 0


def test_adam_counted_rejects_null_counter():
    lib = N.load()
    hp = N.AdamHP(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)
    assert lib.aaa_adam_step_counted(ctypes.byref(hp), None, None, 0, None, None, None, None, None, None, None) == -1


def test_adam_refuses_too_large_tensor_before_the_device():
    """A tensor whose chunks exceed the 2^30 a grid may hold is refused with AAA_E_ARG like every
    other argument, so also on a machine with no device (dummy aligned addresses, never dereferenced)."""
    lib = N.load()
    hp = N.AdamHP(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)
    two = (ctypes.c_void_p * 2)(4096, 4096 + 64)
    for numel, t in (((1 << 43, 7), b"tensor 0"), ((5, 1 << 43), b"tensor 1"), ((1 << 42, 1 << 42), b"tensor 1")):
        rc = lib.aaa_adam_step_counted(ctypes.byref(hp), 4096, None, 2, two, two, two, two, None,
                                       (ctypes.c_size_t * 2)(*numel), None)
        msg = lib.aaa_last_error()
        assert rc == -1 and msg.startswith(b"adam") and b"too large" in msg and t in msg, (rc, msg)


@pytest.mark.parametrize("what,nq,o_ld,q_stride,sq,word", [
    ("o_ld below the 136 the 16-byte loads need", 4, 128, 0, None, b"o_ld"),
    ("o_ld not a multiple of 8", 4, 140, 0, None, b"o_ld"),
    ("sq_scratch with a per-frame query", 4, 192, 4 * 72, 16, b"sq_scratch"),
    ("nq = 5", 5, 192, 0, None, b"nq"),
])
def test_attn_bf16_rejects_bad_args_without_gpu(what, nq, o_ld, q_stride, sq, word):
    """aaa_attn_fwd_bf16 / aaa_attn_bwd_bf16 check their arguments before the
    device: each refusal returns AAA_E_ARG (-1) with a message on a CPU-only box."""
    lib = N.load()
    rc = lib.aaa_attn_fwd_bf16(3, 11, 11, nq, 16, o_ld, 16, 16, q_stride, sq, None, None, 16, 16, None)
    assert rc == -1, what
    assert word in lib.aaa_last_error(), lib.aaa_last_error()
    if sq is None:   # (the backward has no sq_scratch)
        rc = lib.aaa_attn_bwd_bf16(3, 11, 11, nq, 16, o_ld, 16, 16, q_stride, 16, 16, nq * 184, 0, 0, 16, 16, None)
        assert rc == -1, what
        assert word in lib.aaa_last_error(), lib.aaa_last_error()


def test_attn_bwd_bf16_rejects_short_danswer_pitch_without_gpu():
    """da_ld must cover the columns read: nq*184, plus the nq*72 Q columns with add_q."""
    lib = N.load()
    assert lib.aaa_attn_bwd_bf16(3, 11, 11, 4, 16, 192, 16, 16, 0, 16, 16, 4 * 184 - 1, 0, 0, 16, 16, None) == -1
    assert b"da_ld" in lib.aaa_last_error()
    assert lib.aaa_attn_bwd_bf16(3, 11, 11, 4, 16, 192, 16, 16, 0, 16, 16, 4 * 184, 1, 0, 16, 16, None) == -1
    assert b"da_ld" in lib.aaa_last_error()


def test_package_modules_import():
    """Every host module of the package imports on a CPU-only box (no GPU call)."""
    import importlib
    for m in ("learner", "policy", "optim", "parallel", "reinforce", "runtime", "attention"):
        importlib.import_module(f"aaa_amd.{m}")


def test_param_cache_follows_replaced_parameters():
    """Agent._param_list (the per-step parameter list the actor / episode paths
    use) is re-made when a Parameter object is replaced without a registration
    hook or a count change: a direct ``_parameters[k] = ...`` and ``.to()``
    under the overwrite-on-conversion future flag."""
    import torch
    import attention
    a = attention.Agent(num_actions=18)
    ps = a._param_list()
    assert ps == list(a.parameters()) and a._param_list() is ps
    w = a.policy_head[0].weight
    a.policy_head[0]._parameters["weight"] = torch.nn.Parameter(w.detach().clone())
    ps2 = a._param_list()
    assert ps2 is not ps and ps2 == list(a.parameters())
    assert any(p is a.policy_head[0].weight for p in ps2) and not any(p is w for p in ps2)
    prev = torch.__future__.get_overwrite_module_params_on_conversion()
    torch.__future__.set_overwrite_module_params_on_conversion(True)
    try:
        a.double()
        ps3 = a._param_list()
        assert ps3 == list(a.parameters()) and all(p.dtype == torch.float64 for p in ps3)
    finally:
        torch.__future__.set_overwrite_module_params_on_conversion(prev)
