"""Actor-path latency: one environment step of the
reference's Policy.forward (main_mp.py:48-59) at B = 1.

Legs, each over ``--steps`` consecutive steps of one episode (the ConvLSTM
state carries, as in main_mp.py:100), on seeded synthetic uint8 frames:
  policy_item  aaa_amd.policy.Policy.forward: upload uint8 frame, HIP agent
               step, device draw, .item() host sync per step (the reference's
               contract: an int action for env.step)
  policy_async Policy.act: the same without the per-step host sync (one sync at the end)
  graph_item   GraphActor.step: the step captured once as a HIP graph, replayed per
               step, .item() per step (inference / actor-learner split); _chain = the
               actor chain (aaa_actor_step, six small-B launches), _forward = the
               learner's T=1 forward + aaa_sample_actions
  graph_async  GraphActor.step without the per-step sync
  device       graph replays back to back (device time per step, no host copy)
  cpu_ref      the oracle's restatement of the same step (reference op sequence,
               torch CPU fp32, host threads as stated) + softmax/Categorical draw
Prints one JSON line per frame size.  Frames: 210x160 (Seaquest's raw
observation; grid 27x20 = the reference's default SpatialBasis) and 84x84.

``--stateful`` runs the same legs on ``Agent(..., stateful_core=True)`` (the
reference's else branch, attention.py:356-358): _chain is then
aaa_actor_step_core (seven launches), _forward the learner's T=1 stateful
forward, cpu_ref the oracle's stateful step; the record also carries the
zero-state chain's device time from the same process
(``device_chain_zero_state_us``).  ``--reps N`` repeats the device legs N
times in alternation and adds their values (``device_*_reps_us``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import attention  # noqa: E402
from aaa_amd import detinit  # noqa: E402
from aaa_amd.policy import GraphActor, Policy  # noqa: E402


def _device_us(ga, dframe, steps):
    """Device time per step: graph replays back to back on a device-resident frame."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ga.step(dframe)
    ev0.record()
    for t in range(steps):
        ga.graph.replay()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps * 1e3


def gpu_legs(H, W, steps, warmup, dev, stateful=False, reps=1):
    params = detinit.deterministic_params(0, 18, 4)
    agent = attention.Agent(18, grid="auto", stateful_core=stateful)
    detinit.load_into(agent, params)
    agent.to(dev)
    pol = Policy(agent, seed=1)
    frames = detinit.frames_u8(77, (steps + warmup, H, W, 3))
    out = {}
    with torch.no_grad():
        for leg in ("policy_item", "policy_async"):
            agent.reset()
            for t in range(warmup):
                pol(frames[t])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if leg == "policy_item":
                for t in range(steps):
                    pol(frames[warmup + t])
            else:
                for t in range(steps):
                    pol.act(frames[warmup + t])
                torch.cuda.synchronize()
            out[leg] = (time.perf_counter() - t0) / steps * 1e6
            pol.saved_log_probs.clear()
    actors = {}
    for chain in (False, True):
        ga = GraphActor(agent, H, W, B=1, seed=1, chain=chain)
        tag = "chain" if chain else "forward"
        actors[tag] = ga
        for leg in ("graph_item", "graph_async"):
            ga.reset()
            for t in range(warmup):
                int(ga.step(frames[t]).item())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if leg == "graph_item":
                for t in range(steps):
                    int(ga.step(frames[warmup + t]).item())
            else:
                for t in range(steps):
                    ga.step(frames[warmup + t])
                torch.cuda.synchronize()
            out[f"{leg}_{tag}"] = (time.perf_counter() - t0) / steps * 1e6
        dframe = torch.from_numpy(frames[0]).to(dev)
        out[f"device_{tag}"] = _device_us(ga, dframe, steps)
    if stateful:   # the zero-state chain next to it, same process and session
        zero = attention.Agent(18, grid="auto")
        detinit.load_into(zero, params)
        zero.to(dev)
        actors["chain_zero_state"] = GraphActor(zero, H, W, B=1, seed=1, chain=True)
        out["device_chain_zero_state"] = _device_us(actors["chain_zero_state"], dframe, steps)
    if reps > 1:   # the device legs again, alternating (spread of the ratio within one session)
        series = {tag: [] for tag in actors}
        for _ in range(reps):
            for tag, ga in actors.items():
                series[tag].append(round(_device_us(ga, dframe, steps), 1))
        out["reps"] = series
    return out


def cpu_leg(H, W, steps, threads, stateful=False):
    from oracle import ref_cpu
    torch.set_num_threads(threads)
    P = ref_cpu.tensor_params(detinit.deterministic_params(0, 18, 4), requires_grad=False)
    frames = detinit.frames_u8(77, (steps + 1, H, W, 3))
    S = ref_cpu.spatial_basis(*ref_cpu.grid_of(H, W))
    state, core = None, None

    def step(x, state, core):
        out = ref_cpu.unroll(P, x, S=S, state=state, return_state=True, stateful_core=stateful, core_state=core)
        if stateful:
            state, core = out[3]
        else:
            state = out[3]
        return out[0], state, core

    with torch.no_grad():
        # one untimed step, then the timed ones (state carried); frames as main_mp.py:53
        x = torch.from_numpy(frames[0]).float().unsqueeze(0).unsqueeze(0)
        _, state, core = step(x, state, core)
        t0 = time.perf_counter()
        for t in range(1, steps + 1):
            x = torch.from_numpy(frames[t]).float().unsqueeze(0).unsqueeze(0)
            lg, state, core = step(x, state, core)
            probs = torch.softmax(lg[0], dim=-1)                              # main_mp.py:55-58
            dist = torch.distributions.Categorical(probs)
            a = dist.sample()
            dist.log_prob(a)
            int(a.item())
        return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu-steps", type=int, default=20)
    ap.add_argument("--sizes", default="210x160,84x84")
    ap.add_argument("--stateful", action="store_true", help="the stateful policy core (Agent(stateful_core=True))")
    ap.add_argument("--reps", type=int, default=1, help="repeat the device legs this many times, alternating")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    threads = min(16, len(os.sched_getaffinity(0)))
    for sz in args.sizes.split(","):
        H, W = (int(v) for v in sz.split("x"))
        g = gpu_legs(H, W, args.steps, args.warmup, dev, args.stateful, args.reps)
        c = cpu_leg(H, W, args.cpu_steps, threads, args.stateful)
        series = g.pop("reps", None)
        rec = {"metric": "actor step latency (B=1, Policy.forward)", "unit": "us/step", "frame": sz,
               "steps": args.steps, "cpu_ref_us": round(c, 1), "cpu_threads": threads}
        if args.stateful:
            rec["stateful_core"] = True
        rec.update({f"{k}_us": round(v, 1) for k, v in g.items()})
        if series:
            rec.update({f"device_{k}_reps_us": v for k, v in series.items()})
        rec["chain_graph_speedup_vs_cpu"] = round(c / g["graph_item_chain"], 2)
        rec["chain_vs_forward_device"] = round(g["device_forward"] / g["device_chain"], 2)
        print(json.dumps(rec), flush=True)

if __name__ == "__main__":
    main()
