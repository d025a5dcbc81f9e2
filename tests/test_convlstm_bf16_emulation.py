"""CPU evidence for the gates of tests/test_gpu_convlstm_bf16.py (tests/convlstm_bf16_ref.py).

On every case the GPU tests use, correct arithmetic -- the same bf16 operands, fp32
accumulation in two different orders (torch's whole-K, and K in 32-wide tiles summed
one by one), a float32 model of the fast activations, one rounding per store -- must
sit inside (a) / 4, (b), (c) and the CPU share of (d); and each emulated kernel
defect of convlstm_bf16_ref.DEFECTS must break the bound named there.  The
de-permutation of the channel-quad-major slices is checked against an element by
element implementation of the header's maps.

Nothing here touches a device; no kernel is mutated."""
import pytest
import torch

import convlstm_bf16_ref as C

CASES = C.UNROLL_CASES + C.BAND_CASES


def _threads():
    torch.set_num_threads(min(8, torch.get_num_threads()))


@pytest.mark.parametrize("order", ["whole", "tiles"])
@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_fp32_standins_sit_inside_the_bounds(case, order):
    """Both summation orders, both ways the BPTT takes c_t (recomputed from the fp16 gates: the frame-resident
    kernels; stored: the per-step chain -- the second on the whole-K order only)."""
    _threads()
    for ccur in ("recomputed",) + (("stored",) if order == "whole" else ()):
        o = C.standin(case, order, ccur=ccur)
        rep, bad = C.check(o, C.CAP_CPU, a_div=4, what=f"{C.case_id(case)} {order} {ccur}")
        assert not bad, bad
        assert set(rep) == {"c", "gates", "h", "dz", "dx", "dh0", "dc0", "gb", "gb2", "gWx", "gWh"}


@pytest.mark.parametrize("case", C.WGRAD_EDGE_CASES, ids=C.case_id)
def test_fp32_weight_gradient_at_the_k_loop_edges(case):
    """(a) / 4 on gWx, gWh at 75, 363 and 540 pixel rows, both orders."""
    _threads()
    for order in ("whole", "tiles"):
        o = C.standin(case, order)
        assert o["T"] * o["B"] * o["h"] * o["w"] in (75, 363, 540)
        rep, bad = C.check(o, C.CAP_CPU, a_div=4, what=f"{C.case_id(case)} {order}", wgrad_only=True)
        assert not bad, bad
        assert set(rep) == {"gWx", "gWh"}


# the defects on the carried-state 84x84 case (every term of every formula is live there); the stale halo row
# also where it would happen, on the band-mode grid
DEFECT_RUNS = [(d, C.UNROLL_CASES[3]) for d in C.DEFECTS] + [("stale_row", C.BAND_CASES[0])]


@pytest.mark.parametrize("defect,case", DEFECT_RUNS, ids=lambda v: v if isinstance(v, str) else C.case_id(v))
def test_bounds_reject_the_emulated_defects(defect, case):
    _threads()
    order = "tiles" if defect == "splitk_bf16" else "whole"
    o = C.standin(case, order, defect=defect)
    _, bad = C.check(o, C.CAP_DEV, what=f"{C.case_id(case)} {defect}")   # at the DEVICE gates: the wider ones
    failed = {(b, obs) for b, obs, _ in bad}
    assert C.DEFECTS[defect] in failed, (defect, sorted(failed))
    extra = {"trunc_h": ("c", "h"), "border_taps": ("c", "gates"), "stale_row": ("c", "gates"),
             "splitk_bf16": ("a", "gWx")}.get(defect)
    if extra:
        assert extra in failed, (defect, sorted(failed))


@pytest.mark.parametrize("P,B", [(121, 2), (64, 1), (104, 1)])
def test_cqm_depermutation_round_trips(P, B):
    """from_cqm4 / from_cqmg invert a direct, element by element write by include/aaa.h's maps (= csrc/recur.h
    cqm4 / cqmg), per frame, with a leading step dimension."""
    g = torch.Generator().manual_seed(P)
    c = torch.rand((B * P, 128), generator=g)
    gt = torch.rand((B * P, 512), generator=g).to(C.F16)
    assert torch.equal(C.from_cqm4(C.cqm4_direct(c, P), P), c)
    assert torch.equal(C.from_cqmg(C.cqmg_direct(gt, P), P), gt)
    both = torch.stack([C.cqm4_direct(c, P), C.cqm4_direct(c.flip(0), P)])
    assert torch.equal(C.from_cqm4(both, P), torch.stack([c, c.flip(0)]))
    assert not torch.equal(C.cqm4_direct(c, P), c)


def test_single_rounding():
    """rne rounds fp64 once: a value just above a bf16 tie that fp32 would first round onto the tie."""
    y = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8, 0.5 + 2.0 ** -12 + 2.0 ** -40],
                     dtype=torch.float64)
    assert y.float().to(C.BF).double().tolist()[0] == 1.0   # what two roundings give
    assert C.rne(y, C.BF).double().tolist() == [1.0 + 2.0 ** -7, 1.0, 0.5]
    assert C.rne(y, C.F16).double().tolist()[2] == 0.5 + 2.0 ** -11
    assert float(C.ulp_store(torch.tensor([0.3], dtype=torch.float64), C.BF)) == 2.0 ** -9
    assert float(C.ulp_store(torch.tensor([0.75], dtype=torch.float64), C.F16)) == 2.0 ** -11
