"""The fp32 (bf16x6 split products) ConvLSTM weight gradient on the rescheduled
split-at-commit kernel (csrc/gemm.h GemmCfgS6LK through gemm_kernel_s6l,
AAA_WGRAD_S6_PAIRED=1, the default) against the CPU oracle at the fp32
gate (1e-4) and against the parent's loop (AAA_WGRAD_S6_PAIRED=0) in the same
process.

Reference: attention.py:39-102 (ConvLSTMCell: the x- and h-gate convolutions
whose weights these gradients belong to) as used at :119-122, and its autograd
backward; D[512][1728] += dZ^T im2col(XH) with k = the T*B*P pixels.

Shapes are the K loop's edges (rows = T*B*P pixels, BK = 16, min(18, rows / 16)
K splits): less than one tile, exactly one, a partial second tile, odd tile
counts per split, the K tail at 18 splits, tile counts that differ by one
across splits, and the reference's 210x160 frames (27x20 grid: image-row ends
in the im2col gather).

Old-vs-old (selector 0 run twice) and new-vs-old, norm-relative over the 8
ConvLSTM weight gradients, measured on MI355X:
    rows   9, 16, 25 (one split)   0         / 0   (bit for bit)
    rows  75 (3 splits)            1.17e-08  / 3.26e-08
    rows 363 (18 splits)           5.89e-08  / 7.29e-08
    rows 968 (18 splits)           7.52e-08  / 8.76e-08
    rows 540 (18 splits)           6.61e-08  / 7.70e-08
The 75-row case can miss the "twice old-vs-old" bound (2.8 x in the run above)
while far inside the 1e-6 one: a workgroup's partial tile is bit-identical
between the two kernels (every one-split case here; tools/ubench/
wgrad_s6l_ablate.hip checks rows 75, 968 and 77,440 at one split), so what
differs is only the order in which three workgroups' atomics reach an element,
and two runs of one kernel repeat that order more often than runs of two
kernels with different timing.  The bound stays as specified.
"""
import numpy as np
import pytest

from helpers import rel_err
from test_gpu_parity import RTOL, _agent, _compare, _oracle, _run_unroll

import attention

pytestmark = pytest.mark.gpu
N = attention._pkg._native

# (H, W, T, B) -> grid, rows
CASES = [
    (20, 20, 1, 1),     # 3x3, 9 rows: less than one tile, nk == 1
    (28, 28, 1, 1),     # 4x4, 16 rows: exactly one tile
    (36, 36, 1, 1),     # 5x5, 25 rows: two tiles, the second partial, one split
    (36, 36, 3, 1),     # 5x5, 75 rows: odd tile counts within splits
    (84, 84, 3, 1),     # 11x11, 363 rows: 18 splits of one or two tiles, K tail
    (84, 84, 2, 4),     # 11x11, 968 rows: several tiles per split, counts differing by one
    (210, 160, 1, 1),   # 27x20, 540 rows: the reference's frames
]


def _is_lstm_w(name):
    return "vision_lstm.W" in name and name.endswith(".weight")


def _run(cuda, monkeypatch, sel, H, W, T, B, grid):
    monkeypatch.setenv("AAA_WGRAD_S6_PAIRED", sel)
    N.timing_enable(True)
    try:
        out = _run_unroll(_agent(cuda, grid=grid), T, B, cuda, H=H, W=W)
        var = N.timing_stats(N.TIMER_CORE_WGRAD)["variant"]
    finally:
        N.timing_enable(False)
    return out, var


def _flat(g):
    return np.concatenate([g[n].numpy().ravel() for n in sorted(g) if _is_lstm_w(n)])


@pytest.mark.parametrize("H,W,T,B", CASES)
def test_wgrad_paired(cuda, monkeypatch, H, W, T, B):
    from oracle import ref_cpu
    grid = ref_cpu.grid_of(H, W)
    rows = T * B * grid[0] * grid[1]
    what = f"wgrad paired {grid[0]}x{grid[1]} T={T} B={B} ({rows} rows): "
    new, vnew = _run(cuda, monkeypatch, "1", H, W, T, B, grid)
    old, vold = _run(cuda, monkeypatch, "0", H, W, T, B, grid)
    old2, _ = _run(cuda, monkeypatch, "0", H, W, T, B, grid)
    # kernel identity: neither run compares a path with itself
    assert "gemm_kernel_s6l+GemmCfgS6LK" in vnew, vnew
    assert "GemmCfgS6LK" not in vold and "gemm_kernel+" in vold, vold
    assert sum(_is_lstm_w(n) for n in new[3]) == 8
    # against the oracle, every output and gradient
    _compare(new, _oracle(T, B, H=H, W=W), RTOL, what)
    # against the parent's kernel
    a, b, c = _flat(new[3]), _flat(old[3]), _flat(old2[3])
    d_old, d_new = rel_err(c, b), rel_err(a, b)
    print(f"{what}old-vs-old {d_old:.3e}, new-vs-old {d_new:.3e}")
    if rows < 32 and np.array_equal(b, c):
        assert np.array_equal(a, b), what + "one K split: not bit-identical to the parent's kernel"
    else:
        assert d_new <= 2 * d_old, what + f"new-vs-old {d_new:.3e} > 2 x old-vs-old {d_old:.3e}"
        assert d_new <= 1e-6, what + f"new-vs-old {d_new:.3e}"
    # collateral damage: every other gradient and the outputs
    for x, y, n in zip(new[:3], old[:3], ("logits", "values", "attn")):
        assert rel_err(x.numpy(), y.numpy()) <= 1e-5, what + n
    for n in new[3]:
        if not _is_lstm_w(n) and float(old[3][n].norm()) > 0:
            assert rel_err(new[3][n].numpy(), old[3][n].numpy()) <= 1e-5, what + "grad " + n
    assert N.pair_status(clear=True) == 0
