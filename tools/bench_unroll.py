"""Cost of recording actor unrolls on the device, and of starting a learner
unroll from the recorded state (aaa_unroll_begin / aaa_unroll_record,
csrc/unroll.hip; Learner.train_step_vtrace(initial_state=)).

Actor: two GraphActors at B = 16, 84x84, on the fp32 actor chain, in ONE
process -- one as it always was, one with a recorder into a T = 20 collector.
Device time per step as tools/bench_actor.py takes it (graph replays back to
back on a device-resident frame, HIP events), ``--steps`` replays per block so
that a block holds whole unrolls (the boundary steps copy the state: 2 x 62 KB
per row), blocks alternating between the two actors; and the same with the
host in it (GraphActor.step on host frames, with reward and done uploaded for
the recording actor, one sync at the end).

Learner: one C2 learner (B = 32, T = 20, 84x84, fp32, uint8 frames, as
bench.py runs it), lr = 0 so that its weights stay the seeded ones in both
legs, ``train_step_vtrace`` with ``bootstrap="last"`` with and without
``initial_state``, alternating blocks of ``--learner-steps`` iterations.

Median over ``--reps`` blocks.  Prints one JSON line.  No threshold is set.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import attention  # noqa: E402
from aaa_amd import detinit  # noqa: E402
from aaa_amd.learner import Learner  # noqa: E402
from aaa_amd.policy import GraphActor  # noqa: E402
from aaa_amd.unroll import UnrollCollector  # noqa: E402


def device_us(ga, dframe, steps):
    """Device time per step: graph replays back to back on a device-resident frame."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ga.step(dframe)
    ev0.record()
    for _ in range(steps):
        ga.graph.replay()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps * 1e3


def host_us(ga, frames, steps, extras):
    """Host-inclusive time per step: GraphActor.step on host frames, one sync at the end."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        ga.step(frames[t % len(frames)], **extras)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def timed_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def spread(v, m):
    return round(100 * (max(v) - min(v)) / m, 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=190, help="actor steps per block (a multiple of T-1 = 19)")
    ap.add_argument("--learner-steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-learner", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, H, W, A = 16, 20, 84, 84, 18
    agent = attention.Agent(A, grid=(11, 11))
    detinit.load_into(agent, detinit.deterministic_params(0, A, 4))
    agent.to(dev)
    col = UnrollCollector(T, B, H, W, dev)
    actors = {"plain": GraphActor(agent, H, W, B=B, seed=1, chain=True),
              "recording": GraphActor(agent, H, W, B=B, seed=1, chain=True, recorder=col.rows(0, B))}
    frames = detinit.frames_u8(77, (8, B, H, W, 3))
    dframe = torch.from_numpy(frames[0]).to(dev)
    extras = {"plain": {}, "recording": dict(reward=np.ones(B, np.float32), done=np.zeros(B, np.float32))}
    for ga in actors.values():
        device_us(ga, dframe, args.steps)   # warm-up
    dev_us = {k: [] for k in actors}
    hst_us = {k: [] for k in actors}
    for _ in range(args.reps):
        for k, ga in actors.items():
            dev_us[k].append(device_us(ga, dframe, args.steps))
    for _ in range(args.reps):
        for k, ga in actors.items():
            hst_us[k].append(host_us(ga, frames, args.steps, extras[k]))
    dmed = {k: statistics.median(v) for k, v in dev_us.items()}
    hmed = {k: statistics.median(v) for k, v in hst_us.items()}
    state_bytes = 2 * col.state_floats * 4 * B
    out = {"metric": "unroll_recording_cost", "device": torch.cuda.get_device_name(0),
           "actor": {"B": B, "T": T, "frame": f"{H}x{W}", "chain": True, "steps_per_block": args.steps,
                     "blocks": args.reps, "bytes_per_step": 2 * B * H * W * 3,
                     "bytes_per_boundary_step": 2 * state_bytes + B * H * W * 3,
                     "device_us": {k: [round(x, 2) for x in v] for k, v in dev_us.items()},
                     "device_us_median": {k: round(v, 2) for k, v in dmed.items()},
                     "device_block_spread_pct": {k: spread(dev_us[k], dmed[k]) for k in dev_us},
                     "recording_minus_plain_device_us": round(dmed["recording"] - dmed["plain"], 2),
                     "host_step_us_median": {k: round(v, 2) for k, v in hmed.items()},
                     "host_block_spread_pct": {k: spread(hst_us[k], hmed[k]) for k in hst_us},
                     "recording_minus_plain_host_us": round(hmed["recording"] - hmed["plain"], 2)}}
    if not args.no_learner:
        LB = 32
        ln = Learner(LB, T, H, W, 4, A, "fp32", dev, frames_u8=True, lr=0.0)
        r = ln.runner
        lframes = torch.from_numpy(detinit.frames_u8(1234, (T, LB, H, W, 3))).to(dev)
        acts = torch.from_numpy((detinit.frames_u8(5, (T, LB)) % A).astype(np.int32)).to(dev)
        rew = torch.from_numpy((detinit.frames_u8(6, (T, LB)) % 3).astype(np.float32)).to(dev)
        logp = torch.full((T, LB), -float(np.log(A)), device=dev)
        done = torch.zeros(T, LB, device=dev)
        state = (torch.from_numpy(0.1 * detinit.normal(7, r.state_shape())).to(dev),
                 torch.from_numpy(0.1 * detinit.normal(8, r.state_shape())).to(dev))
        kw = dict(bootstrap="last", scale=1.0 / (T * LB))
        legs = {"zero_state": lambda: ln.train_step_vtrace(lframes, acts, rew, logp, done, **kw),
                "initial_state": lambda: ln.train_step_vtrace(lframes, acts, rew, logp, done, initial_state=state, **kw)}
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                ms[k].append(timed_ms(fn, args.learner_steps))
        ln.check_health()
        med = {k: statistics.median(v) for k, v in ms.items()}
        out["learner"] = {"config": "c2", "B": LB, "T": T, "steps_per_block": args.learner_steps, "blocks": args.reps,
                          "lr": 0.0, "updates_applied": ln.opt_steps,
                          "train_step_vtrace_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                          "train_step_vtrace_ms_median": {k: round(v, 4) for k, v in med.items()},
                          "block_spread_pct": {k: spread(ms[k], med[k]) for k in ms},
                          "initial_state_minus_zero_state_ms": round(med["initial_state"] - med["zero_state"], 4),
                          "initial_state_vs_zero_state_pct":
                              round(100 * (med["initial_state"] - med["zero_state"]) / med["zero_state"], 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
