"""Bit-level A/B of the multi-tensor optimizer kernels (csrc/optim.hip): a fixed, seeded
set of Adam, RMSProp and clip cases on whichever library ``AAA_LIB`` names, three steps
each, over the 34 reference tensors plus odd-sized and misaligned ones and over the flat
2,270,276-element buffer.  Prints one JSON line of sha256 digests of every output buffer
(parameters, optimizer state, device step counter, clip stats, scaled gradients) per case.
Run it once per library, each in its own process; there are no atomics in these kernels,
so two libraries that compute the same thing print the same line.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import attention  # noqa: E402,F401
from aaa_amd import _native as N  # noqa: E402
from aaa_amd import detinit  # noqa: E402

CHUNK = 4096   # csrc/optim.hip kAdamChunk
FLAT = 2_270_276
STEPS = 3
INF = float("inf")
REF = [tuple(v.shape) for v in detinit.deterministic_params(0, 18, 4).values()] + [(1,), (3,), (1025,), (7, 9)]
# name -> (shapes, indices put one float off 16-byte alignment: the scalar path)
SETS = {"list": (REF, (3, 30, 36)), "flat": ([(FLAT,)], ())}
CLIP_SETS = {"shapes": (REF, ()), "edge": ([(0,), (CHUNK,), (CHUNK + 1,), (1025,), (2 * CHUNK + 7,)], (3,)),
             "fifty": ([(1 + (i * 37) % 300,) for i in range(49)] + [(CHUNK + 5,)], ()), "flat": ([(FLAT,)], ())}
ADAM = {"plain": dict(lr=1e-3), "decay": dict(lr=3e-3, weight_decay=0.01), "amsgrad": dict(lr=1e-3, amsgrad=True),
        "maximize": dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-6, maximize=True)}
ADAM_MODES = ("host", "counted", "guard0", "guard1", "clip<1", "clip=1", "clip-nonfinite")


def randn(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * (10.0 ** (i % 3 - 1)) for i, s in enumerate(shapes)]


def to_dev(ts, dev, mis):
    out = []
    for i, t in enumerate(ts):
        buf = torch.empty(t.numel() + 1, device=dev)
        v = (buf[1:] if i in mis else buf[:t.numel()]).view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == (4 if i in mis else 0)
        out.append(v)
    return out


def digest(*groups):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for ts in groups:
        for t in ts or ():
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def clip_stats(gs, max_norm, dev):
    stats = torch.empty(4, device=dev)
    scratch = torch.empty(N.grad_norm_scratch_bytes([g.numel() for g in gs]) // 8, dtype=torch.float64, device=dev)
    N.grad_norm(max_norm, gs, stats, scratch)
    return stats


def run(dev, set_name, mode, launch, nstate, seed):
    """Three steps of ``launch(step, ps, gs, states, guard=, step_dev=, clip=)`` in one of ADAM_MODES."""
    shapes, mis = SETS[set_name]
    ps = to_dev(randn(shapes, seed), dev, mis)
    states = [to_dev([torch.zeros(s) for s in shapes], dev, mis) for _ in range(nstate)]
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev) if mode not in ("host", "guard0", "guard1") else None
    guard = torch.tensor([float(mode == "guard1")], device=dev) if mode.startswith("guard") else None
    all_stats = []
    for k in range(STEPS):
        gs = to_dev(randn(shapes, seed + 1 + k), dev, mis)
        if mode == "clip-nonfinite" and k == 1:
            gs[-1].view(-1)[5 % gs[-1].numel()] = INF
        clip = None
        if mode.startswith("clip"):
            clip = clip_stats(gs, 1e30 if mode == "clip=1" else 1e-3, dev)
            all_stats.append(clip)
        launch(k + 1, ps, gs, states, guard=guard, step_dev=step_dev, clip=clip)
    return digest(ps, *states, [step_dev] if step_dev is not None else None, all_stats)


def adam_launch(kw):
    b1, b2 = kw.get("betas", (0.9, 0.999))
    ams = bool(kw.get("amsgrad"))
    hp = N.AdamHP(kw["lr"], b1, b2, kw.get("eps", 1e-8), kw.get("weight_decay", 0.0), int(ams),
                  int(bool(kw.get("maximize"))))

    def launch(step, ps, gs, states, **how):
        N.adam_step(hp, step, ps, gs, states[0], states[1], states[2] if ams else None, **how)
    return launch, 3 if ams else 2


def rmsprop_launch(momentum=0.0, centered=False, eps_in_sqrt=False, weight_decay=0.0, maximize=False, lr_end=0.0,
                   anneal_steps=0):
    hp = N.RmspropHP(1e-3, 0.99, 0.01 if eps_in_sqrt else 1e-8, weight_decay, momentum, lr_end, anneal_steps,
                     int(centered), int(maximize), int(eps_in_sqrt))

    def launch(step, ps, gs, states, **how):
        N.rmsprop_step(hp, step, ps, gs, states[0], states[1] if momentum > 0 else None,
                       states[2] if centered else None, **how)
    return launch, 3


def main():
    dev = torch.device("cuda:0")
    out = {}
    for set_name in SETS:
        for name, kw in ADAM.items():
            launch, nstate = adam_launch(kw)
            for mode in ADAM_MODES:
                out[f"adam/{name}/{mode}/{set_name}"] = run(dev, set_name, mode, launch, nstate, 100)
        for mom in (0.0, 0.9):
            for cent in (False, True):
                for eis in (False, True):
                    launch, nstate = rmsprop_launch(mom, cent, eis)
                    for mode in ("host", "clip<1"):
                        out[f"rmsprop/mom{mom}/cent{int(cent)}/eps_in_sqrt{int(eis)}/{mode}/{set_name}"] = run(
                            dev, set_name, mode, launch, nstate, 200)
        launch, nstate = rmsprop_launch(0.9, True, weight_decay=0.01, maximize=True)
        out[f"rmsprop/decay-maximize/{set_name}"] = run(dev, set_name, "host", launch, nstate, 300)
        launch, nstate = rmsprop_launch(eps_in_sqrt=True, lr_end=1e-4, anneal_steps=2)
        out[f"rmsprop/anneal-counted/{set_name}"] = run(dev, set_name, "counted", launch, nstate, 400)
    for set_name, (shapes, mis) in CLIP_SETS.items():
        gs = to_dev(randn(shapes, 5 + len(shapes)), dev, mis)
        stats = clip_stats(gs, 1.0, dev)
        N.grad_scale(stats, gs)
        out[f"clip/{set_name}"] = digest([stats], gs)
        assert float(stats[1]) < 1.0
    print(json.dumps({"lib": os.path.basename(os.path.dirname(N.LIB_PATH)) + "/" + os.path.basename(N.LIB_PATH),
                      "cases": len(out), "sha256": out}), flush=True)


if __name__ == "__main__":
    main()
