"""The precondition of test_gpu_f32_split.py's split-completeness check, on the
CPU over its whole matrix: for every (case, site, observable) the GPU tests
bound, the error ``e2`` of the quantity with ONE operand of ONE GEMM cut to two
of its three bf16 parts (f32_split_ref.py) is visible (> 0, in fact 1e-6 ..
2e-5), and plain torch float32 evaluation of the same formulas on the same
inputs sits within e2 / 4 -- so a bound of e2 / 2 on a kernel that claims "fp32
accuracy" has a 2x margin on either side: a kernel missing a lo part lands at
about e2, a complete one at fp32 rounding.

The GPU tests evaluate e2 on the kernels' own inputs (their x_t, their saved
gates, the head's dO); the cases here are the same shapes with those inputs
made by the fp32 oracle on the same weights and frames.

Reference: attention.py:110-126 (ConvLSTMCell.forward) and :155-170
(vision_cnn), and their autograd backward.
"""
import pytest
import torch

import f32_split_ref as R

# the figures the issue's emulation reports, with room: e2 in this window is "a lost lo part"
E2_LO, E2_HI = 5e-7, 5e-5


def _check(what, e2, f32, reach):
    for o, sites in reach.items():
        for s in sites:
            if (s, o) not in e2:
                continue
            print(f"{what} {s:>10} -> {o:<4} e2 {e2[s, o]:.3e}  fp32 {f32[o]:.3e}  ratio {f32[o] / e2[s, o]:.3f}")
            assert e2[s, o] > 0, (what, s, o)
            assert E2_LO < e2[s, o] < E2_HI, (what, s, o, e2[s, o])
            assert f32[o] <= e2[s, o] / 4, (what, s, o, f32[o], e2[s, o])


def test_split2_is_two_bf16_parts():
    x = R.rnd((4096,), 7)
    hi = x.to(torch.bfloat16)
    two = R.split2(x)
    err = ((two - x.double()).abs() / x.double().abs().clamp_min(1e-30)).max()
    assert 2.0 ** -20 < float(err) <= 2.0 ** -16   # two round-to-nearest cuts to 8 significand bits: 2^-8 each
    lo = (x - hi.float() - (x - hi.float()).to(torch.bfloat16).float()).to(torch.bfloat16)
    assert torch.equal(two + lo.double(), x.double())   # hi + mid + lo is the fp32 value exactly


def test_layout_round_trips():
    B, h, w = 2, 3, 5
    x = R.rnd((4, B * h * w, 64), 1)
    r = R.to_ref(x, B, h, w)
    assert tuple(r.shape) == (4, B, 64, w, h) and torch.equal(R.from_ref(r), x)
    assert r[1, 1, 7, 4, 2] == x[1, (1 * h + 2) * w + 4, 7]           # pixel (i, j) = (2, 4) of frame 1
    g = R.rnd((B * h * w, 512), 2)
    gr = R.gates_to_ref(g, B, h, w)
    assert tuple(gr.shape) == (B, 4, 128, w, h) and torch.equal(R.gates_from_ref(gr), g)
    assert gr[1, 2, 9, 4, 2] == g[(1 * h + 2) * w + 4, 4 * 9 + 2]     # gate 2 (c~) of channel 9
    flat = R.rnd((4 * (128 * 64 * 9 + 128 + 128 * 128 * 9),), 3)
    assert torch.equal(R.flat_cell_grads(R.split_cell_grads(flat)), flat)


@pytest.mark.parametrize("T,B,H,W,state", R.UNROLL_CASES)
def test_unroll_cases_fp32_within_a_quarter_of_e2(T, B, H, W, state):
    c = R.unroll_case(T, B, H, W, state)
    what = f"T={T} B={B} {H}x{W}{' state' if state else ''}:"
    _check(what + " fwd", c["fwd_e2"], c["fwd_f32"], R.FWD_REACH)
    _check(what + " bwd", c["bwd_e2"], c["bwd_f32"], R.BWD_REACH)
    # what no site is bounded on stays at fp32 rounding
    for o in ("gb", "dc0"):
        assert c["bwd_f32"][o] < 1e-6, (o, c["bwd_f32"][o])


@pytest.mark.parametrize("T,B,H,W,state", R.WGRAD_EDGE_CASES)
def test_wgrad_edge_cases_fp32_within_a_quarter_of_e2(T, B, H, W, state):
    c = R.unroll_case(T, B, H, W, state, R.WGRAD_SITES)
    _check(f"T={T} B={B} {H}x{W}: wgrad", c["bwd_e2"], c["bwd_f32"], R.BWD_REACH)


@pytest.mark.parametrize("B,h,w", R.CELL_CASES)
def test_cell_cases_fp32_within_a_quarter_of_e2(B, h, w):
    c = R.cell_case(B, h, w)
    _check(f"cell {B}x{h}x{w}: fwd", c["fwd_e2"], c["fwd_f32"], R.FWD_REACH)
    _check(f"cell {B}x{h}x{w}: bwd", c["bwd_e2"], c["bwd_f32"], R.BWD_REACH)


@pytest.mark.parametrize("N,H,W", R.CNN_CASES)
def test_cnn_cases_fp32_within_a_quarter_of_e2(N, H, W):
    c = R.cnn_case(N, H, W)
    _check(f"cnn {N}x{H}x{W}:", c["e2"], c["f32"], R.CNN_REACH)


def test_integer_frames_hide_conv1s_input_site():
    """Why the conv1 cases scale their frames: 0..255 integers are exact in bf16."""
    c = R.cnn_case(2, 84, 84)
    W64 = R.cnn_weights()
    x = R.frames(1, 2, 84, 84)[0].permute(0, 3, 2, 1).contiguous()
    ex = R.cnn_pieces(W64, x, c["dy2_ref"])
    cut = R.cnn_pieces(W64, x, c["dy2_ref"], site="conv1.x")
    assert torch.equal(cut["y1"], ex["y1"])
