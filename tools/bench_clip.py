"""Cost of clipping the gradients by global norm in a learner iteration
(aaa_grad_norm + aaa_adam_step_clipped, csrc/optim.hip).

One learner iteration at C2 (B=32, T=20, 84x84, fp32, uint8 frames, as
bench.py runs it) in ONE process and on ONE learner, HIP events on the launch
stream, after warm-up, alternating blocks of ``--steps`` iterations of
Learner.train_step fed precomputed cotangents, three ways:
  none   max_grad_norm=None (the yardstick: the launches as they were)
  off    max_grad_norm huge: the norm is computed, the coefficient is 1
         (the fused Adam takes its unscaled path)
  on     max_grad_norm tiny: the norm is computed and every gradient scaled
and the same three for ``--opt-steps`` back-to-back optimizer_step() calls
alone (the gradients of the last iteration; microseconds per call).
Median of each over ``--reps`` blocks.  Prints one JSON line.
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--opt-steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T, B, A = 20, 32, 18
    lr = Learner(B, T, 84, 84, 4, A, "fp32", dev, frames_u8=True)
    frames = torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3))).to(dev)
    dl = torch.from_numpy(detinit.normal(2, (T, B, A))).to(dev)
    dv = torch.from_numpy(detinit.normal(3, (T, B, A))).to(dev)
    limits = {"none": None, "off": 1e30, "on": 1e-3}

    def train(limit):
        lr.max_grad_norm = limit
        lr.train_step(frames, dl, dv)

    def opt(limit):
        lr.max_grad_norm = limit
        lr.optimizer_step()

    legs = {k: (lambda m=m: train(m)) for k, m in limits.items()}
    opt_legs = {k: (lambda m=m: opt(m)) for k, m in limits.items()}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    us = {k: [] for k in legs}
    coef = {}
    for _ in range(args.reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn, args.steps))
            if k != "none":
                coef[k] = lr.clip_report()["coef"]
    for _ in range(args.reps):
        for k, fn in opt_legs.items():
            us[k].append(1e3 * timed(fn, args.opt_steps))
    lr.check_health()
    assert coef["off"] == 1.0 and coef["on"] < 1.0, coef
    med = {k: statistics.median(v) for k, v in ms.items()}
    umed = {k: statistics.median(v) for k, v in us.items()}

    def spread(v, m):
        return round(100 * (max(v) - min(v)) / m, 2)

    out = {"metric": "grad_clip_cost", "device": torch.cuda.get_device_name(0), "config": "c2", "B": B, "T": T,
           "n_params": lr.runner.n_params, "steps_per_block": args.steps, "opt_steps_per_block": args.opt_steps,
           "blocks": args.reps, "coef": coef,
           "train_step_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "train_step_ms_median": {k: round(v, 4) for k, v in med.items()},
           "train_step_block_spread_pct": {k: spread(ms[k], med[k]) for k in ms},
           "off_vs_none_pct": round(100 * (med["off"] - med["none"]) / med["none"], 2),
           "on_vs_none_pct": round(100 * (med["on"] - med["none"]) / med["none"], 2),
           "optimizer_step_us": {k: [round(x, 2) for x in v] for k, v in us.items()},
           "optimizer_step_us_median": {k: round(v, 2) for k, v in umed.items()},
           "optimizer_step_block_spread_pct": {k: spread(us[k], umed[k]) for k in us},
           "optimizer_off_minus_none_us": round(umed["off"] - umed["none"], 2),
           "optimizer_on_minus_none_us": round(umed["on"] - umed["none"], 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
