"""Actor unrolls recorded on the device (include/aaa.h ``aaa_unroll_begin`` /
``aaa_unroll_record``; csrc/unroll.hip).

An ``UnrollCollector`` owns two banks of time-major unroll buffers in the
layouts ``Learner.train_step_vtrace`` takes.  ``rows(b0, n)`` hands a
``GraphActor`` a recorder for n of their rows; the actor's captured graph then
runs ``begin`` -> step -> ``record`` on every replay, with the write position
in a device-side cursor, so nothing about the graph changes from step to step
and no per-step host work assembles the unroll.  Several actors (the actor
chain stops at B = 16) fill disjoint row ranges of one collector.

Consecutive unrolls share a step: step T-1 of one unroll (whose value is the
V-trace bootstrap, ``bootstrap="last"``) is step 0 of the next.  After n steps
an actor has completed ``0 if n < T else 1 + (n - T) // (T - 1)`` unrolls --
the host knows that from its own count of replays, so ``ready()`` reads
nothing from the device.

    col = UnrollCollector(T=20, B=32, H=84, W=84, device=dev)
    actors = [GraphActor(agent, 84, 84, B=16, seed=s, recorder=col.rows(16 * s, 16)) for s in (0, 1)]
    ...
    for ga, env in zip(actors, envs):
        ga.step(obs, reward, done)          # reward / done: what arrived WITH obs
    if col.ready():
        learner.train_on(col.take())        # views of the finished bank, stream-ordered
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _native as N

__all__ = ["Unroll", "UnrollCollector", "UnrollRows", "completed_unrolls"]


def completed_unrolls(n: int, T: int) -> int:
    """Unrolls of T steps an actor has completed after n steps (consecutive unrolls share one step):
    the value of the device cursor's pos[2], computed on the host."""
    return 0 if n < T else 1 + (n - T) // (T - 1)


class Unroll(NamedTuple):
    """One unroll as ``Learner.train_on`` takes it: frames (T, B, H, W, 3) uint8, actions (T, B) int32,
    rewards / logp / done (T, B) fp32 (row T-1 of rewards and done is zero: ``bootstrap="last"`` reads
    T-1 rows), first (B) fp32 and initial_state = (h0, c0[, core_h0, core_c0]), the state BEFORE step 0."""
    frames: torch.Tensor
    actions: torch.Tensor
    rewards: torch.Tensor
    logp: torch.Tensor
    done: torch.Tensor
    first: torch.Tensor
    initial_state: tuple


class UnrollRows:
    """Recorder of rows [b0, b0 + n) of a collector's banks: what ``GraphActor(recorder=)`` takes.
    Holds the device cursor ``pos`` (4 int32), the static ``reward_in`` / ``done_in`` (n) vectors the
    actor uploads beside the frame, and the host's count of the steps enqueued since ``restart()``."""

    def __init__(self, collector: "UnrollCollector", b0: int, n: int):
        c = collector
        self.collector, self.b0, self.n = c, int(b0), int(n)
        self.pos = torch.zeros(4, dtype=torch.int32, device=c.device)
        self.rd_in = torch.zeros(2, n, device=c.device)   # one buffer, so that one copy uploads both vectors
        self.reward_in, self.done_in = self.rd_in[0], self.rd_in[1]
        self.done_in.fill_(1.0)
        self.steps = 0
        self.fresh = True            # the next step starts an episode in every row (done_in holds ones)
        self.clear = [True, False]   # reward_in / done_in are known to hold zeros
        self.desc = N.UnrollDesc(c.T, n, c.B, b0, c.H * c.W * 3, c.state_floats, 256 if c.stateful_core else 0,
                                 float(c.reward_clip))
        self._live = None

    def attach(self, frame, h, c, core_h=None, core_c=None):
        """The actor's static buffers: this step's frame rows (n, H, W, 3) uint8 and its live state."""
        col = self.collector
        if frame.dtype != torch.uint8 or frame.numel() != self.n * col.H * col.W * 3 or not frame.is_contiguous():
            raise ValueError(f"recorder: the actor's frame buffer must be contiguous uint8 "
                             f"{(self.n, col.H, col.W, 3)}, got {tuple(frame.shape)} {frame.dtype}")
        for name, t, numel in (("h", h, self.n * col.state_floats), ("c", c, self.n * col.state_floats)) + (
                (("core_h", core_h, self.n * 256), ("core_c", core_c, self.n * 256)) if col.stateful_core else ()):
            if t is None or t.dtype != torch.float32 or t.numel() != numel or not t.is_contiguous():
                raise ValueError(f"recorder: {name} must be a contiguous fp32 tensor of {numel} elements "
                                 f"(an actor of {self.n} rows on the collector's grid"
                                 f"{', stateful core' if col.stateful_core else ''})")
        if not col.stateful_core and (core_h is not None or core_c is not None):
            raise ValueError("recorder: the actor carries a policy-core state; build the collector with "
                             "stateful_core=True")
        if frame.device != col.device:
            raise ValueError(f"recorder: the actor is on {frame.device}, the collector on {col.device}")
        self._live = (frame, h, c, core_h, core_c)

    def _io(self, actions=None, logp=None):
        if self._live is None:
            raise RuntimeError("recorder: not attached to an actor (GraphActor(..., recorder=collector.rows(b0, n)))")
        frame, h, c, core_h, core_c = self._live
        io = N.UnrollIO()
        for k, bank in enumerate(self.collector.banks):
            for name in N.UNROLL_BANK_FIELDS:
                setattr(io.bank[k], name, N.ptr(bank[name]))
        for name, t in dict(pos=self.pos, frame=frame, actions=actions, logp=logp, reward_in=self.reward_in,
                            done_in=self.done_in, h=h, c=c, core_h=core_h, core_c=core_c).items():
            setattr(io, name, N.ptr(t))
        return io

    def begin(self):
        """Enqueue aaa_unroll_begin on the current stream (before the actor step)."""
        N.unroll_begin(self.desc, self._io(), N.stream_ptr(self.collector.device))

    def record(self, actions, logp):
        """Enqueue aaa_unroll_record on the current stream (after the actor step): ``actions`` (n) int32
        and ``logp`` (n) fp32 are the step's draw."""
        if actions.dtype != torch.int32 or logp.dtype != torch.float32 or actions.numel() != self.n or \
                logp.numel() != self.n or not actions.is_contiguous() or not logp.is_contiguous():
            raise ValueError(f"recorder: actions must be int32 and logp fp32, contiguous, of {self.n} elements")
        N.unroll_record(self.desc, self._io(actions, logp), N.stream_ptr(self.collector.device))

    def completed(self) -> int:
        """Unrolls this actor has completed (host count; equals the device's pos[2])."""
        return completed_unrolls(self.steps, self.collector.T)

    def episode_start(self):
        """The next step is an episode's first in every row (``GraphActor.reset()``): done_in = 1."""
        self.done_in.fill_(1.0)
        self.fresh, self.clear[1] = True, False

    def restart(self):
        """Start over at step 0 of bank 0: zero the cursor and mark every row an episode start."""
        self.pos.zero_()
        self.reward_in.zero_()
        self.clear[0] = True
        self.steps = 0
        self.episode_start()


class UnrollCollector:
    """Two banks of (T, B, ...) unroll buffers on ``device`` that attached actors fill (module docstring).

    ``reward_clip`` > 0 clamps the recorded rewards to [-c, c] (IMPALA clips to 1); 0 stores them as given.
    ``stateful_core``: the actors carry the policy core's (prev_output, prev_hidden) and the unrolls'
    initial state has four tensors."""

    def __init__(self, T: int, B: int, H: int, W: int, device=None, stateful_core: bool = False,
                 reward_clip: float = 0.0):
        if T < 2:
            raise ValueError(f"UnrollCollector: T must be >= 2 (got {T}): consecutive unrolls share a step")
        if B < 1:
            raise ValueError(f"UnrollCollector: B must be >= 1 (got {B})")
        if not reward_clip >= 0.0:
            raise ValueError(f"UnrollCollector: reward_clip must be >= 0 (got {reward_clip})")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("aaa: the HIP path needs a ROCm GPU tensor device (no CPU fallback)")
        self.T, self.B, self.H, self.W = int(T), int(B), int(H), int(W)
        self.stateful_core, self.reward_clip = bool(stateful_core), float(reward_clip)
        self.h, self.w = N.grid(H, W)
        self.state_floats = self.h * self.w * 128
        self.banks = [self._bank() for _ in range(2)]
        self.handles: list[UnrollRows] = []
        self.taken = 0

    def _bank(self):
        T, B, dev = self.T, self.B, self.device
        state = (B, self.h, self.w, 128)
        bank = dict(frames=torch.zeros(T, B, self.H, self.W, 3, dtype=torch.uint8, device=dev),
                    actions=torch.zeros(T, B, dtype=torch.int32, device=dev),
                    logp=torch.zeros(T, B, device=dev), rewards=torch.zeros(T, B, device=dev),
                    done=torch.zeros(T, B, device=dev), first=torch.zeros(B, device=dev),
                    h0=torch.zeros(state, device=dev), c0=torch.zeros(state, device=dev),
                    core_h0=None, core_c0=None)
        if self.stateful_core:
            bank["core_h0"] = torch.zeros(B, 256, device=dev)
            bank["core_c0"] = torch.zeros(B, 256, device=dev)
        return bank

    def rows(self, b0: int, n: int) -> UnrollRows:
        """A recorder for rows [b0, b0 + n): pass it to ``GraphActor(..., B=n, recorder=)``."""
        if n < 1 or b0 < 0 or b0 + n > self.B:
            raise ValueError(f"UnrollCollector.rows: [{b0}, {b0 + n}) lies outside the collector's {self.B} rows")
        for hd in self.handles:
            if b0 < hd.b0 + hd.n and hd.b0 < b0 + n:
                raise ValueError(f"UnrollCollector.rows: [{b0}, {b0 + n}) overlaps the attached rows "
                                 f"[{hd.b0}, {hd.b0 + hd.n})")
        hd = UnrollRows(self, b0, n)
        self.handles.append(hd)
        return hd

    def ready(self) -> bool:
        """Whether every attached actor has completed an unroll not yet taken (host arithmetic only)."""
        return bool(self.handles) and all(hd.completed() > self.taken for hd in self.handles)

    def take(self, copy: bool = False) -> Unroll:
        """The oldest finished unroll.  ``copy=False``: views of its bank, valid until T-2 further steps
        of any attached actor have been enqueued (the step after those starts rewriting the bank), and
        ordered after the actors' replays on the same stream; ``copy=True``: clones."""
        if not self.ready():
            raise RuntimeError("UnrollCollector.take: no finished unroll (check ready())")
        if any(hd.completed() > self.taken + 1 for hd in self.handles):
            raise RuntimeError("UnrollCollector.take: an actor ran more than one unroll ahead; the finished bank "
                               "has been written again (take() every unroll, or restart())")
        bank = self.banks[self.taken % 2]
        self.taken += 1
        state = (bank["h0"], bank["c0"]) + ((bank["core_h0"], bank["core_c0"]) if self.stateful_core else ())
        u = Unroll(bank["frames"], bank["actions"], bank["rewards"], bank["logp"], bank["done"], bank["first"],
                   state)
        if copy:
            u = Unroll(*(t.clone() for t in u[:6]), tuple(t.clone() for t in state))
        return u

    def restart(self):
        """Drop what has been recorded: every attached actor starts its next step at step 0 of a new
        unroll, as an episode start (pos = 0, done_in = 1)."""
        for hd in self.handles:
            hd.restart()
        self.taken = 0
