"""Evidence that the gates of tests/test_gpu_tail.py mean something, on the CPU:

  * every tail layer computed in float32 the way its kernel orders the sum (16-k
    steps dealt to the tile's wave groups, K slices added one after the other,
    S3 / S6 on real bf16 cuts in the kernel's product order; tail_ref.emulate)
    stays under its bound on every case the GPU test runs, in all three
    arithmetics -- the reference and the bounds alone leave room for a correct
    kernel;
  * each seeded fault breaks a bound on a case the GPU test runs: the ragged
    last K chunk lost in one in-workgroup K slice, a cross product of S3 (lo.hi)
    and of S6 (mid.hi) lost, the bias added once per in-workgroup K slice, a
    ReLU mask taken from row r + 1 at a 32-row tile edge, a weight gradient that
    loses its last F % 256 frames, the [answer | h] operand read at pitch 256.
"""
import numpy as np
import pytest
import torch

import tail_ref as R
from helpers import detinit

_P = {}


def _params(nq, A):
    if (nq, A) not in _P:
        _P[nq, A] = {k: torch.from_numpy(np.asarray(v)).double() for k, v in detinit.deterministic_params(0, A, nq).items()}
    return _P[nq, A]


def _bad(case, arith, fault=None):
    ck = R.check(R.emulate(_params(*case[:2]), case, arith, fault), case, arith)
    print(ck.report())
    return ck.bad


def test_cases_cover_every_reachable_kernel_and_arithmetic():
    assert R.covered() == R.reachable()
    kernels = {k for c in R.CASES for _, k, _, _ in R.plan(*c)["fwd"] + R.plan(*c)["bwd"]}
    assert kernels == {"skinny1", "skinny8", "CFK4", "CF"}
    assert (R.F_LSTM_CF, R.F_ANSWER0_CF, R.F_LSTM_WGRAD_CF) == (705, 1473, 768)


@pytest.mark.parametrize("arith", R.ARITH)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_emulated_kernels_stay_under_the_bounds(case, arith):
    assert not _bad(case, arith)


# fault -> (case of tail_ref.CASES, arithmetic) it must break a bound on
SEEDED = [
    ("ragged", (4, 18, 1, 33, False), "f32"),        # heads dgrad K = 36 and the weight gradients' K = 33: 16-k steps of 4 / 1
    ("ragged", (4, 18, 1, 257, False), "S6"),
    ("cross", (4, 18, 1, 33, False), "S3"),
    ("cross", (4, 18, 1, 33, False), "S6"),
    ("bias_per_slice", (4, 18, 1, 33, False), "S6"),
    ("relu_row", (4, 18, 1, 33, False), "S6"),
    ("relu_row", (8, 5, 1, 8, False), "f32"),
    ("frames256", (4, 18, 1, 257, False), "S6"),
    ("frames256", (4, 18, 1, 520, False), "S3"),
    ("pitch256", (4, 18, 3, 3, True), "S6"),
    ("pitch256", (8, 5, 3, 40, True), "S3"),
]


@pytest.mark.parametrize("fault,case,arith", SEEDED, ids=lambda v: v if isinstance(v, str) else R.case_id(v))
def test_seeded_fault_breaks_a_bound(fault, case, arith):
    assert case in R.CASES and fault in R.FAULTS
    bad = _bad(case, arith, fault)
    assert bad, f"{fault} on {R.case_id(case)} {arith} stayed inside every bound"
    print(bad[:4])


def test_design_table_is_the_restated_dispatch():
    """DESIGN.md "Policy tail: dispatch" is tail_ref.dispatch_markdown(), line for line."""
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    assert R.dispatch_markdown() in text


def test_every_fault_is_seeded():
    assert {f for f, _, _ in SEEDED} == set(R.FAULTS)
