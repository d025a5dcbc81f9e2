"""The recurrence's plan (csrc/rt.h RecurPlan), pinned through the public entries that state it: for a sweep of
dtypes, shapes, flags and one path selector of the environment at a time, aaa_core_layout, aaa_core_elem_bytes,
aaa_workspace_bytes, aaa_packed_bytes and every region of aaa_workspace_region answer what the table under
tests/golden/core_plan.json holds.  The table was recorded from the library of the commit before the plan became
one struct (every reader still deriving it for itself), so it holds for that library and for this one alike.

No GPU needed: without a device the library takes 256 compute units, the MI355X's own count.

Recording (only to add rows; the expected values come from a library known to be right, loaded through AAA_LIB):
    AAA_LIB=<path to libaaa.so> python tests/test_core_plan.py --record
"""
import ctypes
import hashlib
import json
import os
import sys

import pytest

from helpers import ROOT  # noqa: F401  (path setup)

import attention  # noqa: F401
from aaa_amd import _native as N

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "core_plan.json")
DTYPES = {"fp32": N.F32, "bf16": N.BF16}
SHAPES = [(1, 1, 210, 160), (2, 3, 64, 64), (32, 4, 84, 84), (128, 4, 84, 84), (256, 4, 84, 84), (8, 4, 168, 168),
          (64, 4, 168, 168)]
FLAGS = [0, N.FLAG_STATEFUL_CORE, N.FLAG_FRAMES_U8]
# one setting at a time; AAA_BPTT_TILE 6 serves bf16 but reads fp32 gates only (csrc/step_tiles.h: no kG16)
ENVS = ["", "AAA_FUSED_X=0", "AAA_FRAMES_FWD=0", "AAA_FRAMES_FWD=1", "AAA_FRAMES_FWD=2", "AAA_FRAMES_BWD=0",
        "AAA_FRAMES_BWD=2", "AAA_FRAMES_BAND=0", "AAA_F32_FRAMES=0", "AAA_F32_FRAMES=4", "AAA_F32_FRAMES=8",
        "AAA_F32_FRAMES_BWD=0", "AAA_F32_SPLIT6=0", "AAA_BPTT_TILE=6"]
SWEPT = sorted({e.split("=")[0] for e in ENVS if e} | {"AAA_STEP_TILE", "AAA_GATES_F16", "AAA_CQM"})
N_REGIONS = 30   # include/aaa.h enum aaa_ws_region


def _set_env(setting):
    """None of the swept variables but ``setting`` ("NAME=value", or a dict to put back); returns what was set."""
    before = {name: os.environ.pop(name) for name in SWEPT if name in os.environ}
    os.environ.update(dict([setting.split("=")]) if isinstance(setting, str) and setting else setting or {})
    return before


def _row(dtype, shape, flags, setting):
    """What the library answers for one cfg under one environment setting."""
    lib = N.load()
    B, T, H, W = shape
    cfg = N.Cfg(B, T, H, W, 4, 18, DTYPES[dtype], flags)
    before = _set_env(setting)
    try:
        a, b = ctypes.c_int(-1), ctypes.c_int(-1)
        layout = [lib.aaa_core_layout(ctypes.byref(cfg), ctypes.byref(a), ctypes.byref(b)), a.value, b.value]
        a, b = ctypes.c_int(-1), ctypes.c_int(-1)
        elem = [lib.aaa_core_elem_bytes(ctypes.byref(cfg), ctypes.byref(a), ctypes.byref(b)), a.value, b.value]
        regions = []
        for region in range(N_REGIONS):
            off, size = ctypes.c_size_t(0), ctypes.c_size_t(0)
            rc = lib.aaa_workspace_region(ctypes.byref(cfg), region, ctypes.byref(off), ctypes.byref(size))
            regions.append([region, rc, off.value, size.value])
        return {"dtype": dtype, "shape": list(shape), "flags": flags, "env": setting,
                "core_layout": layout, "core_elem_bytes": elem,
                "workspace_bytes": lib.aaa_workspace_bytes(ctypes.byref(cfg)),
                "packed_bytes": lib.aaa_packed_bytes(ctypes.byref(cfg)),
                "regions_sha256": hashlib.sha256(json.dumps(regions).encode()).hexdigest()}
    finally:
        _set_env(before)


def _key(row):
    return (row["dtype"], tuple(row["shape"]), row["flags"], row["env"])


def _table():
    with open(TABLE) as f:
        return {_key(r): r for r in json.load(f)}


@pytest.fixture(scope="module")
def table():
    return _table()


def test_table_covers_the_sweep(table):
    want = {(d, s, f, e) for d in DTYPES for s in SHAPES for f in FLAGS for e in ENVS}
    assert set(table) == want
    # the sweep reaches every kind of plan: both gate sizes, row-major and channel-quad-major slices, no export
    assert {r["core_layout"][1] for r in table.values()} == {2, 4}
    assert {r["core_layout"][2] for r in table.values()} == {0, 7}
    assert {r["core_elem_bytes"][1] for r in table.values()} == {0, 2, 4}


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_plan_matches_the_table(table, dtype, shape, flags):
    for setting in ENVS:
        assert _row(dtype, shape, flags, setting) == table[(dtype, shape, flags, setting)], setting


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: AAA_LIB=<library to record from> python tests/test_core_plan.py --record")
    rows = [_row(d, s, f, e) for d in DTYPES for s in SHAPES for f in FLAGS for e in ENVS]
    with open(TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows from {N.LIB_PATH} -> {TABLE}")
