"""One synchronous learner iteration on the HIP path (bench / DP driver).

step():  pack weights -> T-step forward -> backward (3 phases) with the
gradient buckets all-reduced (RCCL) on a side stream while later work runs.
train_step(): step() followed by the fused Adam update of the flat params
(main_mp.py:78; csrc/optim.hip), i.e. one complete learner iteration.
step() takes its loss cotangents from outside; step_vtrace() /
train_step_vtrace() compute them on the device between the forward and the
backward (V-trace actor-critic, vtrace.py) and share everything else.
Every step method takes ``initial_state``, the recurrent state before step 0
as the actors recorded it (unroll.py), and train_on() runs a whole recorded
unroll; without it an unroll starts from ``reset()``.
Weights live in one flat fp32 buffer in state_dict order, grads likewise, so
a bucket is a contiguous slice and no flatten/unflatten copies are needed.

Co-residency policy: the ConvLSTM recurrence runs as
multi-workgroup frame-resident launches whose partners must all be resident
at once (csrc/common.h launch_resident).  A collective kernel holding CUs
beside them would make partners wait for it, so no all-reduce is in flight
while a forward or a CORE phase is: HEAD's and CORE's buckets are reduced
together once CORE is enqueued (overlapping the VISION phase), VISION's at
the end, and the next step's forward waits for the comm stream.

Stranded-launch guard: one extra fp32 slot after the gradients receives the
partner timeouts reported on this device since the previous step
(aaa_pair_flag: a device-side snapshot of a monotonic word, so no host call
can consume them first) after the CORE phase; it rides in the HEAD+CORE
all-reduce, so every rank sees any rank's timeout, and the fused Adam skips
the update on the device when it is non-zero -- gradients of a stranded
launch never reach the parameters, with no host sync.  The Adam step count
lives on the device too (aaa_adam_step_counted), advanced only by an applied
update, so a skipped step leaves the bias corrections where they were.
``max_grad_norm`` clips the gradients by their global norm inside that update
(aaa_grad_norm, aaa_adam_step_clipped) and skips it the same way when a
gradient is inf or NaN.  ``optimizer="rmsprop"`` puts the fused RMSProp
(aaa_rmsprop_step: IMPALA's optimizer) in Adam's place behind the same guard,
counter and clip; its learning rate anneals over the updates the counter says
were applied, so a skipped step does not move the schedule either.  The
learner's runner defers the API's own stranded check (AAA_FLAG_DEFER_STRANDED):
no rank can raise between its collectives and leave its peers waiting in an
unmatched all-reduce; ``check_health()`` raises after the step instead.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

from . import _native as N
from . import detinit
from .attention import SpatialBasis
from .optim import adam_flat_, rmsprop_flat_, rmsprop_lr
from .parallel import allreduce_buckets, bucket_bounds
from .runtime import UnrollRunner
from .vtrace import episode_starts, vtrace_cotangents


class Learner:
    # IMPALA's RMSProp: no momentum, decay 0.99, eps 0.01 inside the square root (``rmsprop=`` overrides any of them)
    RMSPROP_DEFAULTS = dict(alpha=0.99, eps=0.01, momentum=0.0, centered=False, eps_in_sqrt=True)

    def __init__(self, B: int, T: int, H: int = 84, W: int = 84, nq: int = 4, A: int = 18,
                 dtype: str = "fp32", device=None, seed: int = 0, group=None, lr: float = 1e-3,
                 frames_u8: bool = False, max_grad_norm: float | None = None, optimizer: str = "adam",
                 rmsprop: dict | None = None, lr_anneal_steps: int = 0, lr_end: float = 0.0,
                 stateful_core: bool = False, resets: bool = False):
        # resets: a bf16 learner whose step methods take reset= (UnrollRunner(resets=True)); fp32 learners take it anyway
        if optimizer not in ("adam", "rmsprop"):
            raise ValueError(f"Learner: optimizer must be 'adam' or 'rmsprop' (got {optimizer!r})")
        if optimizer == "adam" and lr_anneal_steps:
            raise ValueError("Learner: lr_anneal_steps needs optimizer='rmsprop' (Adam's lr is constant)")
        if int(lr_anneal_steps) != lr_anneal_steps or lr_anneal_steps < 0 or not 0.0 <= lr_end:
            raise ValueError(f"Learner: lr_anneal_steps must be an integer >= 0 and lr_end >= 0 (got {lr_anneal_steps}, "
                             f"{lr_end})")
        unknown = set(rmsprop or {}) - set(self.RMSPROP_DEFAULTS)
        if unknown:
            raise ValueError(f"Learner: unknown rmsprop setting(s) {sorted(unknown)}; known: "
                             f"{sorted(self.RMSPROP_DEFAULTS)}")
        self.runner = r = UnrollRunner(B, T, H, W, nq, A, dtype, device, stateful_core=stateful_core,
                                       frames_u8=frames_u8, defer_stranded=True, resets=resets)
        self.device = r.device
        params = detinit.deterministic_params(seed, A, nq)
        self.flat = torch.from_numpy(np.concatenate([v.reshape(-1) for v in params.values()])).to(self.device)
        assert self.flat.numel() == r.n_params
        self.packed = r.new_packed()
        self.ws = r.new_workspace()
        # gradients + the stranded-launch guard slot (4 floats: 16-B aligned end)
        self._gbuf = torch.zeros(r.n_params + 4, device=self.device)
        self.grads = self._gbuf[:r.n_params]
        self.guard = self._gbuf[r.n_params:r.n_params + 1]
        # this learner's own snapshot of the device's partner-timeout word (aaa_pair_flag_at): no
        # other reader on the device (another learner, a bench, a diagnostic) can take its timeouts;
        # synced to the current word now, so timeouts from before this learner existed are not its own
        self._pair_base = torch.zeros(1, dtype=torch.int32, device=self.device)
        N.pair_flag(self.guard, base=self._pair_base)
        self._gbuf.zero_()
        self.lr = lr
        self.optimizer = optimizer
        self.lr_anneal_steps, self.lr_end = int(lr_anneal_steps), float(lr_end)
        if optimizer == "adam":
            self.exp_avg = torch.zeros_like(self.grads)
            self.exp_avg_sq = torch.zeros_like(self.grads)
        else:   # only the state the variant uses (aaa_rmsprop_step never touches the rest)
            self.rmsprop = dict(self.RMSPROP_DEFAULTS, **(rmsprop or {}))
            self.square_avg = torch.zeros_like(self.grads)
            self.momentum_buf = torch.zeros_like(self.grads) if self.rmsprop["momentum"] > 0 else None
            self.grad_avg = torch.zeros_like(self.grads) if self.rmsprop["centered"] else None
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.device)   # optimizer updates applied
        # clip by global norm (optimizer_step reads the attribute, so it can be toggled between steps):
        # [norm, coefficient, non-finite flag, max_norm] of the last clipped step, and the norm's partials
        self.max_grad_norm = max_grad_norm
        self.grad_stats = torch.zeros(4, device=self.device)
        self._clip_scratch = None
        if hasattr(N.load(), "aaa_grad_norm"):   # (an older A/B library under AAA_LIB has no clipping entries)
            self._clip_scratch = torch.empty(N.grad_norm_scratch_bytes([r.n_params]) // 8, dtype=torch.float64,
                                             device=self.device)
        self.basis = SpatialBasis(r.h, r.w).S.to(self.device).contiguous()
        self._vt = None   # step_vtrace's (dlogits, dvalues), allocated on its first call
        self.group = group
        self.world =dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        # per-phase gradient ownership (HEAD, CORE, VISION; tools/dp_check.py checks
        # that a phase never writes a range already handed to the all-reduce)
        self.bounds = bucket_bounds(r.offsets, r.n_params)
        n, o_core = r.n_params, self.bounds[1][0]
        # all-reduce schedule: (phase after which it is issued, element ranges of _gbuf)
        self.schedule = {True: [(N.BWD_CORE, [(o_core, n + 1)]), (N.BWD_VISION, [(0, o_core)])],
                         False: [(N.BWD_VISION, [(0, n + 1)])]}
        if self.world > 1:   # identical weights on every rank (they are seeded, but be explicit)
            dist.broadcast(self.flat, src=0, group=group)
            self.comm = torch.cuda.Stream(self.device)   # the gradient all-reduces (RCCL) run here

    def step(self, frames, dlogits, dvalues, overlap: bool = True, comm_timing: bool = False, reset=None,
             initial_state=None):
        """One learner iteration; returns (logits, values).  With N > 1 ranks the
        gradients are SUM-all-reduced over RCCL on a side stream, issued after
        the CORE and VISION phases (``schedule``): the HEAD+CORE reduction
        overlaps the vision backward and never runs beside a frame-resident
        launch.  ``comm_timing`` records per-bucket events; read them with
        comm_stats() after a sync.  ``reset``: None, or a (T, B) episode-start
        mask on the device (``UnrollRunner.forward``; fp32 learners, and bf16
        learners built with ``resets=True``).
        ``initial_state``: None (the unroll starts from ``reset()``), or the
        state before step 0 as the actor held it -- ``(h0, c0)`` (B, h, w, 128),
        with a stateful core ``(h0, c0, core_h0, core_c0)``, the last two
        (B, 256) (``Unroll.initial_state``, unroll.py).  Rows with ``reset[0]``
        start from ``reset()`` whatever it holds (include/aaa.h)."""
        reset = self._reset_mask(reset, None, None)
        logits, values = self._forward(frames, reset, initial_state)
        self._backward(frames, dlogits, dvalues, overlap, comm_timing, reset)
        return logits, values

    def _reset_mask(self, reset, done, first):
        """``reset=`` of the step methods -> None or the (T, B) fp32 device mask: a tensor
        is passed through; "done" is ``episode_starts(done, first)`` over this unroll's T
        steps (``done`` of T, or with bootstrap="last" T-1, rows).  No host read."""
        r = self.runner
        if reset is None:
            if first is not None:
                raise ValueError("first= belongs to reset=\"done\"")
            return None
        if isinstance(reset, str):
            if reset != "done":
                raise ValueError(f"reset must be None, a (T, B) tensor or \"done\", got {reset!r}")
            if done is None:
                raise ValueError("reset=\"done\" needs done")
            d = torch.as_tensor(done).to(device=self.device, dtype=torch.float32).reshape(-1, r.B)
            if d.shape[0] == r.T - 1:   # bootstrap="last" inputs of T-1 rows: the last row starts nothing here
                d = torch.cat([d, torch.zeros(1, r.B, device=self.device)])
            if d.shape[0] != r.T:
                raise ValueError(f"reset=\"done\": done must have {r.T} (or {r.T - 1}) rows, got {d.shape[0]}")
            return episode_starts(d, first)
        if first is not None:
            raise ValueError("first= belongs to reset=\"done\"")
        reset = torch.as_tensor(reset).to(device=self.device, dtype=torch.float32)
        if tuple(reset.shape) != (r.T, r.B):
            raise ValueError(f"reset must be {(r.T, r.B)}, got {tuple(reset.shape)}")
        return reset.contiguous()

    def step_vtrace(self, frames, actions, rewards, behaviour_logp=None, done=None, bootstrap=None,
                    overlap: bool = True, comm_timing: bool = False, reset=None, first=None, initial_state=None,
                    **hparams):
        """One learner iteration on the V-trace actor-critic loss (vtrace.py;
        include/aaa.h ``aaa_vtrace``): pack -> forward -> the loss kernel, from
        this step's own logits / values into the learner's cotangent buffers ->
        the backward, all-reduce schedule and guard of step().  Returns
        (logits, values, loss_parts), loss_parts (B, 3) the raw per-row sums
        ``[-adv log pi[a], (vs - V)^2 / 2, H]``.

        actions (T, B) int32, rewards / behaviour_logp / done (T, B) fp32 and
        bootstrap (B) fp32 should already be contiguous tensors on the learner's
        device (anything else is converted, which copies); behaviour_logp is the
        ``logp`` the actors returned, done and bootstrap as in ``vtrace_loss``
        (``bootstrap="last"`` included: the inputs then have T or T-1 steps'
        worth of rows, of which the first T-1 are used).  ``hparams`` are
        ``vtrace_loss``'s keyword scalars.

        ``reset``: None (the state runs across episode ends, as before), a
        (T, B) episode-start mask, or ``"done"`` = ``episode_starts(done,
        first)``: the step after a ``done`` enters from ``reset()``, and
        ``first`` (B) says which rows start an episode at step 0.  fp32
        learners (include/aaa.h ``aaa_forward_resets``).  ``initial_state``:
        as in step() -- the state the actor held before step 0, so that the
        recomputed log pi is the one ``behaviour_logp`` was drawn under.

        Nothing in the iteration reads the device from the host: there is no
        ``.item()`` and, unlike ``vtrace_loss``, no validation of the action
        range -- an action outside [0, A) makes its row's cotangents NaN (and
        with them the gradients), it reads nothing outside the row.  Under data
        parallelism each rank computes the loss of its own rows and the
        gradients are SUM-all-reduced as in step(); ``scale`` is the caller's
        normalisation (e.g. 1 / (world * B * T))."""
        r = self.runner
        T, B, A = r.T, r.B, r.A
        last = isinstance(bootstrap, str)
        if last and bootstrap != "last":
            raise ValueError(f"bootstrap must be a (B) tensor, None or \"last\", got {bootstrap!r}")
        n = T - 1 if last else T
        if n < 1:
            raise ValueError("bootstrap=\"last\" needs an unroll of at least 2 steps")
        if self._vt is None:   # the loss cotangents: allocated once
            self._vt = (torch.zeros(T, B, A, device=self.device), torch.zeros(T, B, A, device=self.device))
        dl, dv = self._vt

        def dev(x, dtype, sizes):
            if x is None:
                return None
            x = torch.as_tensor(x).to(device=self.device, dtype=dtype).contiguous()
            if x.numel() not in sizes:
                raise ValueError(f"step_vtrace: expected {' or '.join(map(str, sizes))} elements, got {tuple(x.shape)}")
            return x

        tb = (n * B, T * B)   # the kernel reads the first n steps: a contiguous prefix
        actions, rewards = dev(actions, torch.int32, tb), dev(rewards, torch.float32, tb)
        behaviour_logp, done = dev(behaviour_logp, torch.float32, tb), dev(done, torch.float32, tb)
        reset = self._reset_mask(reset, done, first)
        logits, values = self._forward(frames, reset, initial_state)
        if last:
            bootstrap = values[T - 1, :, int(hparams.get("value_col", 0))].contiguous()
            dl[n:].zero_()
            dv[n:].zero_()
        else:
            bootstrap = dev(bootstrap, torch.float32, (B,))
        parts = torch.empty(B, 3, device=self.device)
        vtrace_cotangents(logits, values, actions, rewards, behaviour_logp, done, bootstrap, dl, dv, loss=parts,
                          steps=n, **hparams)
        self._backward(frames, dl, dv, overlap, comm_timing, reset)
        return logits, values, parts

    def _forward(self, frames, reset=None, initial_state=None):
        r = self.runner
        h0 = c0 = core = None
        if initial_state is not None:
            want = 4 if r.stateful_core else 2
            if len(initial_state) != want:
                raise ValueError(f"initial_state must be (h0, c0{', core_h0, core_c0' if want == 4 else ''}) for this "
                                 f"learner, got {len(initial_state)} tensors")
            h0, c0 = initial_state[:2]
            core = tuple(initial_state[2:]) if want == 4 else None
        r.pack(self.flat, self.packed)
        # (a stateful-core runner also returns the core's final state: seven values)
        logits, values = r.forward(self.flat, self.packed, self.basis, frames, self.ws, h0=h0, c0=c0, want_attn=False,
                                   core=core, reset=reset)[:2]
        return logits, values

    def _backward(self, frames, dlogits, dvalues, overlap, comm_timing, reset=None):
        """The backward half of an iteration: the three phases into ``grads``,
        the all-reduce schedule and the stranded-launch guard."""
        r = self.runner
        if self.world == 1:
            r.backward(self.flat, self.packed, self.basis, frames, self.ws, dlogits, dvalues, grads=self.grads,
                       reset=reset)
            N.pair_flag(self.guard, base=self._pair_base)
            return
        main = torch.cuda.current_stream(self.device)
        self._events = [] if comm_timing else None
        issue = dict(self.schedule[bool(overlap)])
        for phase in (N.BWD_HEAD, N.BWD_CORE, N.BWD_VISION):
            r.backward(self.flat, self.packed, self.basis, frames, self.ws, dlogits, dvalues, grads=self.grads,
                       phases=phase, reset=reset)
            if phase == N.BWD_CORE:   # every resident launch of this step is enqueued by now
                N.pair_flag(self.guard, base=self._pair_base)
            if phase in issue:
                self._allreduce(main, issue[phase], comm_timing)
        if comm_timing:
            self._compute_done = torch.cuda.Event(enable_timing=True)
            self._compute_done.record(main)
        main.wait_stream(self.comm)

    def _allreduce(self, main, bounds, timing):
        ready = torch.cuda.Event(enable_timing=timing)
        ready.record(main)                          # everything the phase enqueued
        with torch.cuda.stream(self.comm):
            self.comm.wait_event(ready)
            for lo, hi in bounds:
                t0 = torch.cuda.Event(enable_timing=True) if timing else None
                if timing:
                    t0.record(self.comm)
                allreduce_buckets(self._gbuf, [(lo, hi)], self.group, async_op=False)
                if timing:
                    t1 = torch.cuda.Event(enable_timing=True)
                    t1.record(self.comm)
                    self._events.append((lo, hi, ready, t0, t1))

    def comm_stats(self):
        """Per-bucket all-reduce time (ms) and the communication left exposed
        after the last backward phase (ms) of the last timed step()."""
        if not getattr(self, "_events", None):
            raise RuntimeError("comm_stats(): the last step() ran without comm_timing=True (or on one rank)")
        o_core, n = self.bounds[1][0], self.runner.n_params
        names = {(o_core, n + 1): "HEAD+CORE (+guard)", (0, o_core): "VISION", (0, n + 1): "ALL (+guard)"}
        buckets = []
        for lo, hi, ready, t0, t1 in self._events:
            buckets.append({"bucket": names.get((lo, hi), f"[{lo},{hi})"), "bytes": 4 * (hi - lo),
                            "allreduce_ms": round(t0.elapsed_time(t1), 4),
                            "queued_after_phase_ms": round(ready.elapsed_time(t0), 4)})
        last = self._events[-1][4]
        exposed = max(0.0, self._compute_done.elapsed_time(last))
        return {"buckets": buckets, "exposed_ms": round(exposed, 4),
                "policy": "no collective beside a frame-resident launch: HEAD+CORE reduced after CORE, VISION last"}

    @property
    def opt_steps(self) -> int:
        """Optimizer updates applied so far (reads the device counter: syncs)."""
        return int(self.step_dev.item())

    def check_health(self):
        """Raise if a frame-resident launch of ANY rank timed out waiting for a
        partner in the last step (syncs the stream).  The decision is the guard
        slot, which the HEAD+CORE all-reduce summed over the ranks, so every rank
        sees the same value and all ranks raise together -- none goes on into the
        next step's collective while a peer has left.  The host-side
        count is consumed too (it would otherwise fail the next API call of this
        process); the guarded Adam has already refused the step's update."""
        g = float(self.guard.item())
        n = N.pair_status(clear=True)
        if g != 0.0 or n:
            raise RuntimeError(f"aaa: {int(g)} partner wait(s) of a frame-resident launch timed out on the "
                               f"ranks ({n} on this one); the step's optimizer update was skipped on every rank")

    def optimizer_step(self):
        """Adam (lr=1e-3, torch defaults; main_mp.py:92) on the flat params, one
        launch, skipped on the device when the guard slot is non-zero (and then
        not counted: the device step counter advances only on an update).

        With ``max_grad_norm`` set, the gradients are first clipped by their
        global 2-norm, on the device: the norm of ``grads`` (under data
        parallelism the SUM-all-reduced ones -- _backward has made this stream
        wait for the comm stream; the guard slot is not part of it) goes to
        ``grad_stats``, and the update runs on ``grads * coefficient`` inside
        the same fused launch.  A norm that is not finite -- some gradient
        element is inf or NaN -- skips the update exactly as the guard does.

        ``optimizer="rmsprop"``: the same launches with the fused RMSProp
        (aaa_rmsprop_step) in Adam's place -- the guard, the device step counter
        and the clip stats are passed alike, and the learning rate follows its
        linear anneal over the updates the counter says were applied."""
        clip = None
        if self.max_grad_norm is not None:
            if self._clip_scratch is None:
                raise RuntimeError("aaa: the loaded library has no aaa_grad_norm (an older build under AAA_LIB); "
                                   "max_grad_norm needs it -- there is no fallback")
            N.grad_norm(self.max_grad_norm, [self.grads], self.grad_stats, self._clip_scratch,
                        stream=N.stream_ptr(self.device))
            clip = self.grad_stats
        if self.optimizer == "rmsprop":
            rmsprop_flat_(self.flat, self.grads, self.square_avg, 0, momentum_buf=self.momentum_buf,
                          grad_avg=self.grad_avg, guard=self.guard, step_dev=self.step_dev, clip=clip, lr=self.lr,
                          lr_end=self.lr_end, anneal_steps=self.lr_anneal_steps, **self.rmsprop)
        else:
            adam_flat_(self.flat, self.grads, self.exp_avg, self.exp_avg_sq, 0, lr=self.lr, guard=self.guard,
                       step_dev=self.step_dev, clip=clip)

    def current_lr(self) -> float:
        """The learning rate the next update will use: the anneal at ``opt_steps`` (constant for
        Adam and without ``lr_anneal_steps``).  Reads the device counter: syncs; for logging,
        outside the iteration."""
        if self.optimizer != "rmsprop":
            return float(self.lr)
        return rmsprop_lr(self.opt_steps, self.lr, self.lr_end, self.lr_anneal_steps)

    def clip_report(self) -> dict:
        """The last clipped step's norm, coefficient, non-finite flag and
        max_norm (reads the device: syncs; for logging, outside the iteration)."""
        norm, coef, bad, mx = self.grad_stats.tolist()
        return {"norm": norm, "coef": coef, "nonfinite": int(bad), "max_norm": mx}

    def train_step(self, frames, dlogits, dvalues, overlap: bool = True, reset=None, initial_state=None):
        out = self.step(frames, dlogits, dvalues, overlap=overlap, reset=reset, initial_state=initial_state)
        self.optimizer_step()
        return out

    def train_step_vtrace(self, frames, actions, rewards, behaviour_logp=None, done=None, bootstrap=None,
                          overlap: bool = True, reset=None, first=None, initial_state=None, **hparams):
        """step_vtrace() followed by the fused Adam update: a complete learner
        iteration, stream-ordered, with no host round trip."""
        out = self.step_vtrace(frames, actions, rewards, behaviour_logp, done, bootstrap, overlap=overlap,
                               reset=reset, first=first, initial_state=initial_state, **hparams)
        self.optimizer_step()
        return out

    def train_on(self, unroll, **hparams):
        """One complete iteration on an unroll the actors recorded
        (``UnrollCollector.take()``, unroll.py): train_step_vtrace() on its
        buffers with ``bootstrap="last"``, from the state the actors held before
        its step 0.  fp32 learners, and bf16 learners built with ``resets=True``,
        also cut the state at the episode ends inside it (``reset="done"`` with
        the unroll's ``first``); other bf16 learners refuse a reset mask and get
        the initial state alone (its rows of ``first`` hold the reset() state
        already: the recorder stores the state after the episode-start reset)."""
        if self.runner.dtype == "fp32" or self.runner.resets:
            hparams = dict(hparams, reset="done", first=unroll.first)
        return self.train_step_vtrace(unroll.frames, unroll.actions, unroll.rewards, unroll.logp, unroll.done,
                                      bootstrap="last", initial_state=unroll.initial_state, **hparams)
