"""CPU evidence for the gates of tests/test_gpu_vision_bf16.py (tests/vision_bf16_ref.py).

On every case the GPU tests use, correct arithmetic -- the same bf16 operands,
fp32 accumulation in two different orders, one rounding to bf16 -- must sit well
inside the gates, and three emulated kernel faults must each break one:

  * conv1's output truncated to bf16 instead of rounded,
  * one pixel row dropped from conv2's weight-gradient sum,
  * a border row of the Y1 image not zero (a copy of the map's first row).

Nothing here touches a device; no kernel is mutated."""
import functools

import pytest
import torch

import vision_bf16_ref as R

BF = R.BF
CASES = R.cpu_cases()


@functools.lru_cache(maxsize=4)
def _case(H, W, N, src):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    H1, W1, h, w = R.geometry(H, W)
    xp = R.xp_expected(R.frames(H, W, N, src))
    y1_64, S1 = R.conv1_ref(xp)
    y1a, y1b = R.conv1_f32_orders(xp)
    y1k = y1a.to(BF)   # the operand every later product reads
    dy2 = R.cot_dy2(N, h * w).reshape(N, h, w, 64)
    return dict(H1=H1, W1=W1, h=h, w=w, xp=xp, y1_64=y1_64, S1=S1, y1a=y1a, y1b=y1b, y1k=y1k, dy2=dy2)


def _ids(c):
    return f"{c[0]}x{c[1]}-{c[2]}-{c[3]}"


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fp32_orders_sit_inside_the_forward_bounds(case):
    """(b) and (c) for Y1, the conv2 output and dY1 on two fp32 summation orders."""
    c = _case(*case)
    x2_64, S2 = R.conv2_ref(c["y1k"])
    d_64, SD = R.dgrad_ref(c["dy2"], c["H1"], c["W1"])
    sets = (("y1", (c["y1a"], c["y1b"]), c["y1_64"], c["S1"], R.K1),
            ("x2", R.conv2_f32_orders(c["y1k"]), x2_64, S2, R.K2),
            ("dy1", R.dgrad_f32_orders(c["dy2"], c["H1"], c["W1"]), d_64, SD, R.KD))
    for name, orders, y64, S, K in sets:
        for i, y32 in enumerate(orders):
            k = y32.to(BF)
            ratio, ulps = R.bound_b(k, y64, S, K)
            ok, share = R.share_ok(k, y64, R.MISMATCH_CPU)
            print(f"{_ids(case)} {name} order {i}: bound ratio {ratio:.3f}, worst {ulps:.3f} ulp, mismatch {share:.2e}")
            assert ratio <= 1.0, (name, i, ratio)
            assert ok, (name, i, share)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fp32_gradients_sit_inside_a_quarter_of_the_gates(case):
    """(d) and (e): fp32 weight gradients in two orders, at a quarter of the device gates."""
    c = _case(*case)
    N = case[2]
    xp, y1k, dy2 = c["xp"], c["y1k"], c["dy2"]
    g2_64 = R.gw2_ref(y1k, dy2)
    g2 = (R.gw2_ref(y1k, dy2, torch.float32),
          R.per_frame_sum(lambda n: R.gw2_ref(y1k[n:n + 1], dy2[n:n + 1], torch.float32), N))
    d32a, _ = R.dgrad_f32_orders(dy2, c["H1"], c["W1"])
    dk = d32a.to(BF)
    g1_64 = R.gw1_ref(xp, dk)
    g1 = (R.gw1_ref(xp, dk, torch.float32),
          R.per_frame_sum(lambda n: R.gw1_ref(xp[n:n + 1], dk[n:n + 1], torch.float32), N))
    g1_own, e_flip = R.fused_gw1_ref(xp, dy2, c["H1"], c["W1"])
    for i in range(2):
        e2, e1, ee = R.rel(g2[i], g2_64), R.rel(g1[i], g1_64), R.rel(g1[i], g1_own)
        print(f"{_ids(case)} order {i}: gW2 {e2:.2e} gW1 {e1:.2e} gW1 vs own-dY1 ref {ee:.2e} (e_flip {e_flip:.2e})")
        assert e2 <= R.GATE_W / 4 and e1 <= R.GATE_W / 4, (i, e2, e1)
        assert ee <= (4 * e_flip + 1e-5) / 4, (i, ee, e_flip)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_emulated_faults_break_a_bound(case):
    c = _case(*case)
    y1k, dy2 = c["y1k"], c["dy2"]
    # 1. truncation instead of rounding: half the elements are no longer bf16(y64)
    kt = R.trunc_bf16(c["y1a"])
    ratio, _ = R.bound_b(kt, c["y1_64"], c["S1"], R.K1)
    ok, share = R.share_ok(kt, c["y1_64"], R.MISMATCH_CAP)
    assert ratio > 1.0 or not ok, (ratio, share)
    # 2. one pixel row (the last frame's last pixel) dropped from conv2's weight gradient
    drop = dy2.clone()
    drop[-1, -1, -1, :] = 0
    e = R.rel(R.gw2_ref(y1k, drop, torch.float32), R.gw2_ref(y1k, dy2))
    assert e > R.GATE_W, e
    # 3. a non-zero border row of the Y1 image
    x2_64, S2 = R.conv2_ref(y1k)
    kb = R.conv2_f32_orders(y1k, pad_fault=True)[0].to(BF)
    ratio, _ = R.bound_b(kb, x2_64, S2, R.K2)
    assert ratio > 1.0, ratio
    print(f"{_ids(case)}: truncation share {share:.2f}, dropped pixel {e:.2e}, border ratio {ratio:.1f}")


def test_bf16_rne_is_one_rounding():
    """The reference's own rounding: exact ties go to even, and a value that fp32 would first round
    onto a tie still rounds by its fp64 distance."""
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8 - 2.0 ** -40),
                      0.0, 2.0 ** -8], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, 2.0 ** -8], dtype=torch.float64)
    assert torch.equal(R.bf16_rne(t).double(), want)
    u = R.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.75, -3.0], dtype=torch.float64))
    assert torch.equal(u, torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6], dtype=torch.float64))
