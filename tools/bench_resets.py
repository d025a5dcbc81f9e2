"""Cost of episode-start masks in a learner iteration (aaa_forward_resets /
aaa_backward_resets, csrc/resets.hip).

One learner iteration at C2 (B=32, T=20, 84x84, fp32, uint8 frames, as
bench.py runs it; ``--config c3``: B=256, T=20, bf16, a learner built with
``resets=True``) in ONE process and on ONE learner, HIP events on the launch
stream, after warm-up, alternating blocks of ``--steps`` iterations of
Learner.train_step fed precomputed cotangents, three ways:
  none   reset=None (the yardstick: the frame-group / frame-resident kernels)
  zero   an all-zero (T, B) mask (the mask variants, no row cut)
  one    one reset per row at a seeded step in [1, T)
and with ``--config c3`` a fourth leg in a child process:
  steps  the same one-reset mask with AAA_FRAMES_FWD=0 AAA_FRAMES_BWD=0 (the
         per-step chains in both directions)
Median ms per iteration of each over ``--reps`` blocks.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--config", choices=("c2", "c3"), default="c2")
    ap.add_argument("--only", default=None, help="(the steps leg's child) time this mask alone, report it as 'steps'")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T, B, A = (20, 32, 18) if args.config == "c2" else (20, 256, 18)
    if args.config == "c2":
        lr = Learner(B, T, 84, 84, 4, A, "fp32", dev, frames_u8=True)
    else:
        lr = Learner(B, T, 84, 84, 4, A, "bf16", dev, frames_u8=True, resets=True)
    frames = torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3))).to(dev)
    dl = torch.from_numpy(detinit.normal(2, (T, B, A))).to(dev)
    dv = torch.from_numpy(detinit.normal(3, (T, B, A))).to(dev)
    g = torch.Generator().manual_seed(args.seed)
    one = torch.zeros(T, B)
    one[torch.randint(1, T, (B,), generator=g), torch.arange(B)] = 1.0
    masks = {"none": None, "zero": torch.zeros(T, B, device=dev), "one": one.to(dev)}
    if args.only:
        masks = {"steps": masks[args.only]}
    legs = {k: (lambda m=m: lr.train_step(frames, dl, dv, reset=m)) for k, m in masks.items()}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn, args.steps))
    lr.check_health()
    if args.only:   # the child: its blocks alone
        print(json.dumps({"ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}}), flush=True)
        return
    if args.config == "c3":   # the per-step chains under the same mask, in a fresh process (the plan reads the environment)
        env = dict(os.environ, AAA_FRAMES_FWD="0", AAA_FRAMES_BWD="0")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", "c3", "--only", "one", "--steps",
                                str(args.steps), "--reps", str(args.reps), "--warmup", str(args.warmup), "--seed",
                                str(args.seed)], env=env, check=True, capture_output=True, text=True, timeout=600)
        ms.update(json.loads(child.stdout.strip().splitlines()[-1])["ms"])
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"metric": "reset_mask_cost", "device": torch.cuda.get_device_name(0), "config": args.config, "B": B, "T": T,
           "steps_per_block": args.steps, "blocks": args.reps,
           "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "zero_vs_none_pct": round(100 * (med["zero"] - med["none"]) / med["none"], 2),
           "one_vs_zero_pct": round(100 * (med["one"] - med["zero"]) / med["zero"], 2),
           "none_block_spread_pct": round(100 * (max(ms["none"]) - min(ms["none"])) / med["none"], 2)}
    if "steps" in med:
        out["one_vs_steps_pct"] = round(100 * (med["one"] - med["steps"]) / med["steps"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
