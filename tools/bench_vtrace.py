"""Cost of the V-trace actor-critic loss (csrc/loss.hip, aaa_vtrace) on the device.

Two measurements, HIP events on the launch stream, after warm-up:
  kernel  device time per aaa_vtrace launch, ``--launches`` launches back to
          back between one event pair, at the C2 (T=20, B=32), C3 (20, 256) and
          C5-per-GPU (50, 64) shapes, A = 18, every optional input and output
          set; median / min / max over ``--reps`` such batches
  step    one learner iteration at C2 (B=32, T=20, 84x84, fp32, uint8 frames,
          as bench.py runs it) in ONE process and on ONE learner, alternating
          blocks of ``--steps`` iterations: Learner.train_step fed precomputed
          cotangents (the yardstick: what the learner did before it owned a
          loss) against Learner.train_step_vtrace; median ms per iteration of
          each over ``--reps`` blocks, and their difference
Prints one JSON line.
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
from aaa_amd.vtrace import vtrace_cotangents  # noqa: E402

SHAPES = {"c2": (20, 32, 18), "c3": (20, 256, 18), "c5_per_gpu": (50, 64, 18)}


def loss_inputs(T, B, A, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    mu = torch.log_softmax(torch.randn(T, B, A, generator=g) * 3, -1)
    actions = torch.randint(0, A, (T, B), generator=g, dtype=torch.int32)
    x = dict(actions=actions, rewards=(torch.rand(T, B, generator=g) < 0.2).float(),
             behaviour_logp=mu.gather(-1, actions.long().unsqueeze(-1)).squeeze(-1).contiguous(),
             done=(torch.rand(T, B, generator=g) < 0.05).float(), bootstrap=torch.randn(B, generator=g))
    return {k: v.to(dev) for k, v in x.items()}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n   # ms


def kernel_leg(shape, dev, launches, reps, warmup):
    T, B, A = shape
    g = torch.Generator().manual_seed(1)
    lg, vl = (torch.randn(T, B, A, generator=g) * 3).to(dev), torch.randn(T, B, A, generator=g).to(dev)
    x = loss_inputs(T, B, A, dev)
    dl, dv = torch.empty_like(lg), torch.empty_like(vl)
    vs, adv, parts = torch.empty(T, B, device=dev), torch.empty(T, B, device=dev), torch.empty(B, 3, device=dev)

    def launch():
        vtrace_cotangents(lg, vl, x["actions"], x["rewards"], x["behaviour_logp"], x["done"], x["bootstrap"],
                          dl, dv, vs, adv, parts)

    timed(launch, warmup)
    us = [timed(launch, launches) * 1e3 for _ in range(reps)]
    return {"T": T, "B": B, "A": A, "us_per_launch_median": round(statistics.median(us), 3),
            "us_per_launch_min": round(min(us), 3), "us_per_launch_max": round(max(us), 3),
            "bytes_moved": 4 * (4 * T * B * A + 6 * T * B + 4 * B)}   # 4 (T,B,A) arrays, 6 (T,B), bootstrap + parts


def step_leg(dev, steps, reps, warmup):
    T, B, A = SHAPES["c2"]
    lr = Learner(B, T, 84, 84, 4, A, "fp32", dev, frames_u8=True)
    frames = torch.from_numpy(detinit.frames_u8(1234, (T, B, 84, 84, 3))).to(dev)
    dl = torch.from_numpy(detinit.normal(2, (T, B, A))).to(dev)
    dv = torch.from_numpy(detinit.normal(3, (T, B, A))).to(dev)
    x = loss_inputs(T, B, A, dev)
    hp = dict(scale=1.0 / (T * B))

    def parent():
        lr.train_step(frames, dl, dv)

    def vtrace():
        lr.train_step_vtrace(frames, **x, **hp)

    for _ in range(max(1, warmup // 2)):
        parent()
        vtrace()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(parent, steps))
        b.append(timed(vtrace, steps))
    lr.check_health()
    ma, mb = statistics.median(a), statistics.median(b)
    return {"config": "c2", "B": B, "T": T, "steps_per_block": steps, "blocks": reps,
            "train_step_ms": [round(v, 4) for v in a], "train_step_vtrace_ms": [round(v, 4) for v in b],
            "train_step_ms_median": round(ma, 4), "train_step_vtrace_ms_median": round(mb, 4),
            "difference_us": round((mb - ma) * 1e3, 2), "difference_pct_of_parent": round(100 * (mb - ma) / ma, 3),
            "parent_block_spread_pct": round(100 * (max(a) - min(a)) / ma, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="kernel legs only")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "vtrace_loss_cost", "device": torch.cuda.get_device_name(0),
           "kernel": {k: kernel_leg(s, dev, args.launches, args.reps, args.warmup) for k, s in SHAPES.items()}}
    if not args.no_step:
        out["step"] = step_leg(dev, args.steps, args.reps, args.warmup)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
