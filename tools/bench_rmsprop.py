"""Cost of the fused RMSProp beside the fused Adam in a learner iteration
(aaa_rmsprop_step / aaa_adam_step_counted, csrc/optim.hip).

Four learners at C2 (B=32, T=20, 84x84, fp32, uint8 frames, as bench.py runs
it) in ONE process, HIP events on the launch stream, after warm-up,
alternating blocks:
  adam      Learner() as it is by default
  impala    optimizer="rmsprop": momentum 0, alpha 0.99, eps 0.01 inside the
            root, lr annealed -- 12 B read + 8 B written per element against
            Adam's 16 + 12
  momentum  the same with momentum 0.9 (one more buffer: 16 + 12)
  clipped   impala with max_grad_norm tiny: the norm launches, every gradient scaled
``--opt-steps`` back-to-back optimizer_step() calls alone (the gradients of the
last iteration; microseconds per call) and ``--steps`` iterations of
Learner.train_step fed precomputed cotangents.  Median of each over ``--reps``
blocks.  Prints one JSON line.

The learning rate is 0 by default: every kernel moves the same bytes, but the
weights stay the seeded ones in all four learners.  The time of the forward
and backward depends on the weights (with ``--lr 1e-3`` the learners drift
apart and their train_step differs by several per cent while their
optimizer_step differs by microseconds), so learners that train cannot be
compared by train_step.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import attention  # noqa: E402,F401
from aaa_amd import detinit  # noqa: E402
from aaa_amd.learner import Learner  # noqa: E402


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n   # ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--opt-steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.0,
                    help="0 (default): the kernels move the same bytes but every learner stays at the seeded weights")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T, B, A = 20, 32, 18
    anneal = 10 ** 9   # never reached here: the schedule is evaluated on the device all the same
    kw = dict(H=84, W=84, nq=4, A=A, dtype="fp32", device=dev, frames_u8=True, lr=args.lr)
    learners = {
        "adam": Learner(B, T, **kw),
        "impala": Learner(B, T, optimizer="rmsprop", lr_anneal_steps=anneal, **kw),
        "momentum": Learner(B, T, optimizer="rmsprop", rmsprop=dict(momentum=0.9), lr_anneal_steps=anneal, **kw),
        "clipped": Learner(B, T, optimizer="rmsprop", lr_anneal_steps=anneal, max_grad_norm=1e-3, **kw),
    }
    frames = torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3))).to(dev)
    dl = torch.from_numpy(detinit.normal(2, (T, B, A))).to(dev)
    dv = torch.from_numpy(detinit.normal(3, (T, B, A))).to(dev)
    w0 = learners["adam"].flat.clone()   # the seeded initial weights, the same in every learner
    legs = {k: (lambda ln=ln: ln.train_step(frames, dl, dv)) for k, ln in learners.items()}
    opt_legs = {k: ln.optimizer_step for k, ln in learners.items()}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    us = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn, args.steps))
    for _ in range(args.reps):
        for k, fn in opt_legs.items():
            us[k].append(1e3 * timed(fn, args.opt_steps))
    coef = learners["clipped"].clip_report()["coef"]
    steps = {k: ln.opt_steps for k, ln in learners.items()}
    for ln in learners.values():
        ln.check_health()
    assert coef < 1.0, coef
    assert len(set(steps.values())) == 1, steps   # every update of every learner was applied
    med = {k: statistics.median(v) for k, v in ms.items()}
    umed = {k: statistics.median(v) for k, v in us.items()}

    def spread(v, m):
        return round(100 * (max(v) - min(v)) / m, 2)

    n = learners["adam"].runner.n_params
    bytes_per_elem = {"adam": 28, "impala": 20, "momentum": 28, "clipped": 20 + 4}   # clipped: + the norm's read
    out = {"metric": "rmsprop_cost", "device": torch.cuda.get_device_name(0), "config": "c2", "B": B, "T": T,
           "n_params": n, "steps_per_block": args.steps, "opt_steps_per_block": args.opt_steps, "blocks": args.reps,
           "lr": args.lr, "weights_moved": {k: not torch.equal(w0, ln.flat) for k, ln in learners.items()},
           "clip_coef": coef, "updates_applied": steps["adam"], "bytes_per_element": bytes_per_elem,
           "optimizer_step_us": {k: [round(x, 2) for x in v] for k, v in us.items()},
           "optimizer_step_us_median": {k: round(v, 2) for k, v in umed.items()},
           "optimizer_step_block_spread_pct": {k: spread(us[k], umed[k]) for k in us},
           "optimizer_step_gbps_median": {k: round(n * bytes_per_elem[k] / (umed[k] * 1e-6) / 1e9, 1) for k in umed},
           "impala_minus_adam_us": round(umed["impala"] - umed["adam"], 2),
           "momentum_minus_adam_us": round(umed["momentum"] - umed["adam"], 2),
           "clipped_minus_impala_us": round(umed["clipped"] - umed["impala"], 2),
           "train_step_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "train_step_ms_median": {k: round(v, 4) for k, v in med.items()},
           "train_step_block_spread_pct": {k: spread(ms[k], med[k]) for k in ms},
           "train_step_vs_adam_pct": {k: round(100 * (med[k] - med["adam"]) / med["adam"], 2) for k in med}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
