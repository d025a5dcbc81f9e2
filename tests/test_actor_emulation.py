"""Evidence that the gates of tests/test_gpu_actor_pins.py mean something, on the CPU:

  * every stage of the actor chain computed in float32 in its kernel's own
    partition (conv1's four K quarters, conv2's lanes along K, the ConvLSTM's
    six K slices, 16-position readout chunks with the max / sum merge, clamped
    float4 slices per lane and the butterfly; actor_ref.emulate) stays under
    its bound on every case the GPU test runs, with no allowance -- the
    reference and the bounds alone leave room for a correct kernel;
  * each seeded single mistake (actor_ref.FAULTS) breaks the bound of the stage
    it was seeded into on a case the GPU test runs;
  * the checker's view of the workspace (aaa_actor_workspace_region) lies
    inside the workspace, 256-byte aligned and without overlap, and is refused
    exactly where the step is.
"""
import ctypes
import os

import pytest
import torch

import actor_ref as R
import f32_split_ref as SR
from helpers import ROOT

import attention  # noqa: F401
from aaa_amd import _native as N


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_emulated_stages_stay_under_the_bounds(case):
    o = R.emulate(case)
    ck = R.check(o, case, "emulated")
    print(ck.report())
    assert not ck.bad, ck.bad
    if case[2] <= 5 and R.geom(case)["P"] <= 121:   # a second, chained step from the first one's state
        ck = R.check(R.emulate(case, step=1, state=R.next_state(case, o)), case, "emulated step 1")
        assert not ck.bad, ck.bad


_BY_ID = {R.case_id(c): c for c in R.CASES}
# fault -> (a case of actor_ref.CASES, the stage whose bound it must break there)
SEEDED = [
    ("conv1_pad_clamped", "84x84_B16nq4A256_u8_oop", "vision"),
    ("conv1_pad_clamped", "8x8_B4nq8A1_core_f32_noprev", "vision"),
    ("conv2_ring_bias", "210x160_B1nq8A18_core_u8_oop", "vision"),
    ("conv2_ring_bias", "16x16_B1nq4A3_core_u8_oop", "vision"),
    ("convlstm_slice_dropped", "64x64_B5nq4A18_core_u8_noprev_oop", "convlstm.gates"),
    ("convlstm_slice_dropped", "506x256_B1nq8A18_u8_noprev", "convlstm.gates"),
    ("convlstm_pad_pixel0", "8x8_B5nq4A3_u8_oop", "convlstm.gates"),
    ("convlstm_pad_pixel0", "84x84_B16nq8A256_core_f32", "convlstm.gates"),
    ("readout_clamped_rows_weighted", "84x84_B16nq4A256_u8_oop", "answer row"),   # P % 16 = 9
    ("readout_clamped_rows_weighted", "16x16_B4nq8A17_f32", "answer row"),        # P = 4
    ("merge_first_64_chunks", "264x256_B1nq8A18_f32_oop", "answer row"),          # nch = 66
    ("merge_first_64_chunks", "506x256_B1nq4A18_core_f32_oop", "map"),            # nch = 128
    ("merge_own_max", "64x64_B1nq8A17_f32", "answer row"),
    ("merge_own_max", "256x256_B1nq4A18_u8", "map"),
    ("prev_swapped", "84x84_B16nq8A256_core_f32", "answer row"),
    ("clamped_slice_twice", "16x16_B1nq4A3_core_u8_oop", "query4"),               # K = 288: lanes 8.. clamp to 284
    ("clamped_slice_twice", "84x84_B16nq8A256_core_f32", "query2"),               # K = 128: lanes 32.. clamp to 124
    ("heads_pad_row_wraps", "8x8_B4nq8A1_core_f32_noprev", "heads"),              # 2A = 2
    ("heads_pad_row_wraps", "16x16_B4nq8A17_f32", "heads"),                       # 2A = 34: a 2-row last group
    ("lstm_gate_major", "8x8_B5nq4A3_u8_oop", "lstm.h"),
    ("lstm_gate_major", "210x160_B1nq8A18_core_u8_oop", "lstm.c"),
    ("lstm_fc_dropped", "64x64_B5nq4A18_core_u8_noprev_oop", "lstm.c"),
    ("h_copy_last_share", "210x160_B4nq4A18_f32_noprev", "h carry"),
    ("h_copy_last_share", "8x8_B5nq4A3_u8_oop", "h carry"),
]


@pytest.mark.parametrize("fault,case,stage", SEEDED, ids=lambda v: v)
def test_seeded_fault_breaks_a_bound(fault, case, stage):
    assert fault in R.FAULTS and case in _BY_ID
    c = _BY_ID[case]
    ck = R.check(R.emulate(c, fault), c, fault)
    assert ck.bad, f"{fault} on {case} stayed inside every bound"
    assert any(b.startswith(stage + ":") for b in ck.bad), (stage, ck.bad)
    print(ck.bad[:4])


def test_every_fault_is_seeded():
    assert {f for f, _, _ in SEEDED} == set(R.FAULTS)


def test_answer0_clamped_slice_is_the_zero_padding():
    """Why clamped_slice_twice is shown on the query MLP and not on answer.0: k_act_ans0's clamped last slice
    [ans_ld - 4, ans_ld) lies wholly in the row's zero padding (ans_ld - ans_in = 6 at nq = 4 and 8), so counting it
    again adds exact zeros; the answer row check holds that padding to exactly 0."""
    for nq in (4, 8):
        g = R.geom((84, 84, 1, nq, 18, False, True, True, False))
        assert g["ans_ld"] - 4 >= g["ans_in"] and g["ans_ld"] <= 256 * R.nit_ans0(nq)
        assert 256 * (R.nit_ans0(nq) - 1) < g["ans_ld"]


def test_convlstm_statement_is_the_shared_recurrence():
    """actor_ref's gate pre-activations, pushed through tail_ref's gate / cell functions, are f32_split_ref.recur_fwd
    (the fp64 recurrence every ConvLSTM pin shares) on the same operands -- layouts and gate order included."""
    c = _BY_ID["16x16_B4nq8A17_f32"]
    g = R.geom(c)
    raw, _ = R.params(c[3], c[4])
    B, P, hw = g["B"], g["P"], (g["h"], g["w"])
    X, st = R.rnd(1, (B, P, 64), 2.0), R.state0(c)
    gates, _ = R.convlstm_gates(raw, X, st["h"], hw)
    cc, _ = R.convlstm_c(gates, st["c"])
    hh, _ = R.convlstm_h(gates, cc)
    ref = SR.recur_fwd(SR.cell_weights(raw), SR.to_ref(X.double().reshape(B * P, 64), B, *hw)[None],
                       SR.to_ref(st["h"].double().reshape(B * P, 128), B, *hw),
                       SR.to_ref(st["c"].double().reshape(B * P, 128), B, *hw))
    assert float((SR.gates_from_ref(ref["gates"][0]) - gates.reshape(B * P, 512)).abs().max()) < 1e-13
    assert float((SR.from_ref(ref["c"][0]) - cc.reshape(B * P, 128)).abs().max()) < 1e-13
    assert float((SR.from_ref(ref["h"][0]) - hh.reshape(B * P, 128)).abs().max()) < 1e-13


# ---------------------------------------------------- the region entry --------
def _cfg(c, **kw):
    H, W, B, nq, A, core, u8 = c[:7]
    d = dict(B=B, T=1, H=H, W=W, nq=nq, A=A, dtype=N.F32,
             flags=(N.FLAG_STATEFUL_CORE if core else 0) | (N.FLAG_FRAMES_U8 if u8 else 0))
    d.update(kw)
    return N.Cfg(d["B"], d["T"], d["H"], d["W"], d["nq"], d["A"], d["dtype"], d["flags"])


def _region(cfg, r):
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    rc = N.load().aaa_actor_workspace_region(ctypes.byref(cfg), r, ctypes.byref(off), ctypes.byref(nb))
    return rc, off.value, nb.value


def _ws_bytes(cfg):
    lib = N.load()
    core = bool(cfg.flags & N.FLAG_STATEFUL_CORE)
    return (lib.aaa_actor_core_workspace_bytes if core else lib.aaa_actor_workspace_bytes)(ctypes.byref(cfg))


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_regions_tile_the_workspace(case):
    """Offsets 256-byte aligned, sizes as include/aaa.h states them, every region inside the workspace of the
    chain the cfg's flag selects, no two overlapping; _QT / _Q1 / _Q2 only with the stateful core."""
    cfg, g, core = _cfg(case), R.geom(case), case[5]
    B, P, nq = g["B"], g["P"], g["nq"]
    want = {"X": B * P * 64, "HS": B * P * 128, "HID1": B * 512, "AO": B * 256, "LH": B * 256, "LOGITS": B * P * nq,
            "ANSWER": B * g["ans_ld"], "QT": B * g["qd"], "Q1": B * 128, "Q2": B * g["qd"]}
    total = _ws_bytes(cfg)
    assert total > 0 and total % 256 == 0
    spans = []
    for name, r in N.ACT_WS.items():
        rc, off, nb = _region(cfg, r)
        if name in ("QT", "Q1", "Q2") and not core:
            assert rc == -1 and b"region" in N.load().aaa_last_error()
            continue
        assert rc == 0 and off % 256 == 0 and nb == 4 * want[name] and off + nb <= total, (name, rc, off, nb, total)
        spans.append((off, off + nb))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    for unknown in (-1, len(N.ACT_WS)):
        assert _region(cfg, unknown)[0] == -1


def test_regions_refused_exactly_where_the_step_is():
    """AAA_E_ARG for every cfg aaa_actor_step / aaa_actor_step_core refuses (their workspace queries return 0):
    bf16, T > 1, B > 16, grids past kActMaxChunks chunks (65x32 = 130 chunks, 64x64), nq = 5; granted,
    following AAA_FLAG_STATEFUL_CORE, wherever a workspace exists.  NULL arguments are refused."""
    lib = N.load()
    base = (84, 84, 1, 4, 18, False, True)
    assert N.grid(514, 256) == (65, 32) and N.grid(506, 256) == (64, 32)
    for flags in (0, N.FLAG_STATEFUL_CORE, N.FLAG_FRAMES_U8 | N.FLAG_STATEFUL_CORE):
        for kw, ok in ((dict(), True), (dict(B=16), True), (dict(H=506, W=256), True), (dict(dtype=N.BF16), False),
                       (dict(T=2), False), (dict(B=17), False), (dict(H=514, W=256), False),
                       (dict(H=506, W=506), False), (dict(nq=5), False)):
            cfg = _cfg(base, flags=flags, **kw)
            assert (_ws_bytes(cfg) > 0) == ok, kw
            for r in N.ACT_WS.values():
                granted = ok and (r < N.ACT_WS["QT"] or bool(flags & N.FLAG_STATEFUL_CORE))
                assert (_region(cfg, r)[0] == 0) == granted, (kw, flags, r)
                assert granted or _region(cfg, r)[0] == -1
    cfg = _cfg(base)
    off = ctypes.c_size_t()
    assert lib.aaa_actor_workspace_region(None, 0, ctypes.byref(off), ctypes.byref(off)) == -1
    assert lib.aaa_actor_workspace_region(ctypes.byref(cfg), 0, None, ctypes.byref(off)) == -1
    assert lib.aaa_actor_workspace_region(ctypes.byref(cfg), 0, ctypes.byref(off), None) == -1


def test_binding_matches_header_enum():
    import re
    src = open(os.path.join(ROOT, "include", "aaa.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"AAA_ACT_WS_([A-Z0-9]+)\s*=\s*(\d+)", src)}
    assert enum == N.ACT_WS and sorted(enum.values()) == list(range(10))


def test_design_n_table_is_the_one_the_bounds_use():
    """DESIGN.md "Actor chain: accuracy on its own operands" holds actor_ref.n_table, line for line."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert n_table_markdown() in text


def n_table_markdown():
    a, b = R.n_table(4, 121), R.n_table(8, 2048)
    rows = ["| stage | n (nq = 4, P = 121) | n (nq = 8, P = 2048) |", "|---|---|---|"]
    rows += [f"| {k} | {a[k]} | {b[k]} |" for k in a]
    return "\n".join(rows)


def test_tau_exp_is_four_times_the_measurement():
    assert R.TAU_EXP == min(4 * R.TAU_EXP_MEASURED, R.TAU_CAP) and R.TAU_EXP <= R.TAU_CAP
    assert torch.isfinite(torch.tensor(R.POISON))
