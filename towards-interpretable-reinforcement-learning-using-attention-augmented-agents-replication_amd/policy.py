"""Actor path on the device: the reference's ``Policy``.

``Policy`` mirrors main_mp.py:40-59 -- same constructor, attributes
(``agent``, ``saved_log_probs``, ``rewards``) and ``forward(observation, ts=0)
-> int`` -- so ``train``/``finish_episode`` (main_mp.py:62-80, 95-150) and
test_model.py:42-73 run unchanged with it.  What changes underneath:

* the observation goes to the GPU as uint8 (1/4 of the float bytes the
  reference copies at main_mp.py:53) and is cast inside the kernel that lays
  the frames out for conv1 (AAA_FLAG_FRAMES_U8);
* the agent step is the HIP forward (``Agent.forward``, T=1), whose packed
  weights are cached between parameter updates (``Agent._packed_params``);
* softmax, the Categorical draw and its log-prob are one kernel
  (``aaa_sample_actions``, csrc/loss.hip) with a device-side draw counter, so
  ``act()`` returns the action as a device tensor without a host sync; only
  ``forward`` calls ``.item()``, as the reference does at main_mp.py:59.

The saved log-probs are differentiable through the per-step agent graph, so
``torch.cat(policy.saved_log_probs)`` in finish_episode back-propagates into
the hand-written BPTT exactly like the reference's Categorical objects.
Sampling uses its own counter-based generator (not torch's multinomial
stream): the same distribution, different draws.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _native as N

__all__ = ["Policy", "sample_actions", "ActionSampler", "GraphActor"]


def _sample_raw(logits, seed, counter):
    """aaa_sample_actions on (B, A) fp32 logits -> (actions int32 (B,), log_prob (B,),
    jac (B, A) = d log_prob / d logits); no autograd."""
    B, A = logits.shape
    lg = logits.detach().contiguous()
    actions = torch.empty(B, dtype=torch.int32, device=lg.device)
    logp = torch.empty(B, dtype=torch.float32, device=lg.device)
    jac = torch.empty(B, A, dtype=torch.float32, device=lg.device)
    N.check(N.load().aaa_sample_actions(B, A, lg.data_ptr(), int(seed) & (2**64 - 1),
                                        None if counter is None else counter.data_ptr(),
                                        actions.data_ptr(), logp.data_ptr(), jac.data_ptr(),
                                        N.stream_ptr(lg.device)), "sample_actions")
    return actions, logp, jac


class _SampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, seed, counter):
        actions, logp, jac = _sample_raw(logits, seed, counter)
        ctx.save_for_backward(jac)
        ctx.mark_non_differentiable(actions)
        return actions, logp

    @staticmethod
    def backward(ctx, _g_actions, g_logp):
        (jac,) = ctx.saved_tensors
        return jac * g_logp.unsqueeze(1), None, None


def sample_actions(logits: torch.Tensor, seed: int = 0, counter: torch.Tensor | None = None):
    """Draw one action per row of ``logits`` (B, A) from softmax(logits).

    Returns ``(actions int32 (B,), log_prob (B,))``; ``log_prob`` is
    differentiable w.r.t. ``logits`` (d/dl_k = 1[k = a] - p_k).  ``counter``
    is a device int64 scalar tensor advanced by one per call (None: draw 0).
    """
    if logits.dim() != 2:
        raise ValueError(f"logits must be (B, A), got {tuple(logits.shape)}")
    if not logits.is_cuda or logits.dtype != torch.float32:
        raise RuntimeError("sample_actions: logits must be fp32 on the gfx950 device (there is no CPU fallback)")
    if counter is not None and (counter.dtype != torch.int64 or counter.numel() != 1 or
                                counter.device != logits.device):
        raise ValueError("counter must be a one-element int64 tensor on the logits' device")
    return _SampleFn.apply(logits, seed, counter)


class ActionSampler:
    """A seeded draw stream on one device: ``sampler(logits) -> (actions, log_prob)``."""

    def __init__(self, seed: int = 0, device=None):
        self.seed = int(seed)
        self.counter = torch.zeros(1, dtype=torch.int64, device=device if device is not None else "cuda")

    def __call__(self, logits):
        if self.counter.device != logits.device:
            self.counter = self.counter.to(logits.device)
        return sample_actions(logits, self.seed, self.counter)


class Policy(nn.Module):
    """main_mp.py:40-59 on the gfx950 path (see the module docstring)."""

    def __init__(self, agent, seed: int | None = None):
        super().__init__()
        self.agent = agent
        self.saved_log_probs = []
        self.rewards = []
        if seed is None:   # follow torch.manual_seed(config.seed + rank) (main_mp.py:87) like the reference's draws
            seed = int(torch.initial_seed())
        self._sampler = None
        self._seed = seed
        self._frames = []      # ring of (pinned uint8 staging buffer, copy-done event)
        self._slot = 0

    def _device(self):
        # the agent's cached parameter list as last validated (the device of its first
        # parameter: .to() moves parameters in place), without re-validating it -- the
        # step's _episode_params does that once per step
        c = getattr(self.agent, "__dict__", {}).get("_plist")
        if c is not None and c[3]:
            return c[3][0].device
        pl = getattr(self.agent, "_param_list", None)
        return pl()[0].device if pl is not None else next(self.agent.parameters()).device

    def _upload(self, observation):
        dev = self._device()
        if isinstance(observation, torch.Tensor):
            x = observation.to(dev, non_blocking=True)
        else:
            obs = np.ascontiguousarray(observation)
            src = torch.from_numpy(obs)
            if obs.dtype == np.uint8:   # stage through pinned memory: async H2D of 1 B/pixel
                if not self._frames or self._frames[0][0].shape != src.shape:
                    self._frames = [(torch.empty(src.shape, dtype=torch.uint8, pin_memory=True),
                                     torch.cuda.Event()) for _ in range(4)]
                buf, done = self._frames[self._slot]
                self._slot = (self._slot + 1) % len(self._frames)
                done.synchronize()      # the copy that last read this buffer (4 steps ago) has finished
                buf.copy_(src)
                x = buf.to(dev, non_blocking=True)
                done.record(torch.cuda.current_stream(dev))
                return x.unsqueeze(0)           # uint8: cast inside the frame-layout kernel
            x = src.to(dev)
        return (x if x.dtype == torch.uint8 else x.float()).unsqueeze(0)

    def act(self, observation, ts: int = 0):
        """One step without a host sync: returns (action int32 (1,), log_prob (1,)) on the device."""
        state = self._upload(observation)
        dev = state.device
        if self._sampler is None or self._sampler.counter.device != dev:
            self._sampler = ActionSampler(self._seed, dev)
        act_episode = getattr(self.agent, "act_episode", None)
        out = act_episode(state, self._sampler, ts=ts) if act_episode is not None else None
        if out is not None:   # the step and its draw as ONE episode node (episode.py _EpisodeActFn)
            action, logp = out
        else:
            logits, _ = self.agent(state, ts=ts)
            action, logp = self._sampler(logits)
        self.saved_log_probs.append(logp)
        return action, logp

    def forward(self, observation, ts: int = 0):
        """Sample an action from the agent's output distribution (main_mp.py:48-59)."""
        action, _ = self.act(observation, ts)
        return int(action.item())


def _actor_chain_fits(B, H, W, nq, A, stateful_core: bool = False) -> bool:
    """Whether aaa_actor_step (aaa_actor_step_core for the stateful policy
    core) accepts this geometry: its layout query returns 0 bytes (AAA_E_ARG)
    for what it refuses, e.g. a grid whose readout exceeds the kernel's LDS;
    no device call."""
    import ctypes
    cfg = N.Cfg(B, 1, H, W, nq, A, N.F32, N.FLAG_FRAMES_U8 | (N.FLAG_STATEFUL_CORE if stateful_core else 0))
    lib = N.load()
    query = lib.aaa_actor_core_workspace_bytes if stateful_core else lib.aaa_actor_workspace_bytes
    return query(ctypes.byref(cfg)) > 0


class GraphActor:
    """One B-row environment step of the agent + action draw, captured once as
    a HIP graph and replayed per step (inference: test_model.py rollouts, or
    the acting half of an actor/learner split whose learner re-runs the
    episode with ``Agent.unroll`` + ``reinforce_loss``).

    ``step(observation)`` -> action int32 (B,) device tensor (the draw of
    Policy.forward, main_mp.py:54-57), with ``logits``, ``values``,
    ``log_prob`` and ``attention`` left in static device buffers.  The
    ConvLSTM state carries between steps inside the graph (``reset()`` zeroes
    it, attention.py:293-296).  For an agent with ``stateful_core`` the policy
    core's (prev_output, prev_hidden) carry the same way, in ``core_h`` /
    ``core_c`` (B, 256), and the queries follow them step by step
    (attention.py:324-331, 356-358).  Weights are re-packed into the graph's own
    buffers whenever a parameter of ``agent`` changed (storage or in-place
    version), so optimizer steps between episodes are picked up.

    ``chain`` selects the step: the actor chain (``aaa_actor_step``: six
    launches sized for small B, or ``aaa_actor_step_core``: seven, for the
    stateful policy core; fp32 agents, B <= 16) or the learner's T=1 forward
    (``aaa_forward`` + ``aaa_sample_actions``: bf16 agents, larger B or grids);
    None picks the chain whenever it applies.

    ``recorder`` (``UnrollCollector.rows(b0, B)``, unroll.py) adds two calls
    to the captured step -- ``aaa_unroll_begin`` before it, ``aaa_unroll_record``
    after it, on either path -- that reset the rows whose episode ended and
    write the step into the collector's time-major unroll buffers at a
    device-side cursor; ``step`` then also takes the reward and done flag that
    came with the observation.  Without one the captured launches are the
    step's alone.
    """

    def __init__(self, agent, H: int, W: int, B: int = 1, seed: int = 0, chain: bool | None = None, recorder=None):
        from .runtime import ActorRunner, UnrollRunner
        self.agent = agent
        dev = next(agent.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("GraphActor needs the agent on the gfx950 device (there is no CPU fallback)")
        self.device, self.B, self.H, self.W = dev, B, H, W
        self.stateful = bool(getattr(agent, "stateful_core", False))
        eligible = agent.conv_dtype == "fp32" and B <= 16
        if chain and not eligible:
            raise ValueError("the actor chain needs an fp32 agent and B <= 16 (bf16 agents and larger batches act "
                             "through the learner's T=1 forward: chain=False)")
        self.chain = eligible if chain is None else bool(chain)
        if self.chain and chain is None and not _actor_chain_fits(B, H, W, agent.num_queries, agent.num_actions,
                                                                  self.stateful):
            self.chain = False   # the geometry the chain refuses (its readout LDS): the learner's T=1 forward
        if self.chain:   # any failure here (asked for, or a real HIP error) propagates
            r = ActorRunner(B, H, W, agent.num_queries, agent.num_actions, dev, frames_u8=True,
                            stateful_core=self.stateful)
        if self.chain:
            self.runner = r
            self._ws = r.new_workspace()
            A = agent.num_actions
            self._logits = torch.empty(B, A, device=dev)
            self._values = torch.empty(B, A, device=dev)
            self._attn = torch.empty(B, r.h, r.w, agent.num_queries, device=dev)
            self._actions = torch.empty(B, dtype=torch.int32, device=dev)
            self._logp = torch.empty(B, device=dev)
        else:
            r = UnrollRunner(B, 1, H, W, agent.num_queries, agent.num_actions, agent.conv_dtype, dev,
                             stateful_core=self.stateful, frames_u8=True)
            self.runner = r
        self.S = agent._basis_for(r.h, r.w, H, W, dev)
        self.params = list(agent.parameters())
        self.flat = torch.empty(r.n_params, device=dev)
        self.packed = r.new_packed()
        self._key = None
        self.frame_u8 = torch.zeros(1, B, H, W, 3, dtype=torch.uint8, device=dev)
        self.h = torch.zeros(r.state_shape(), device=dev)
        self.c = torch.zeros(r.state_shape(), device=dev)
        # the policy core's (prev_output, prev_hidden): carried inside the graph like h / c
        self.core_h = torch.zeros(B, 256, device=dev) if self.stateful else None
        self.core_c = torch.zeros(B, 256, device=dev) if self.stateful else None
        self.sampler = ActionSampler(seed, dev)
        self._host = [(torch.empty(B, H, W, 3, dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
                      for _ in range(4)]
        self._slot = 0
        self.recorder = recorder
        if recorder is not None:   # the unroll recorder's two calls ride in the captured step (unroll.py)
            if recorder.n != B:
                raise ValueError(f"GraphActor: the recorder holds {recorder.n} rows, the actor steps {B}")
            recorder.attach(self.frame_u8, self.h, self.c, self.core_h, self.core_c)
            # reward / done staging beside the frame ring: (pinned (2, B) fp32, its numpy view)
            self._host_rd = [(t, t.numpy()) for t in (torch.zeros(2, B, pin_memory=True) for _ in self._host)]
        self._refresh()
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream), torch.no_grad():
            for _ in range(2):      # warm-up outside the capture (lazy library init, allocator)
                self._body()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=stream):
                self._outs = self._body()
        torch.cuda.current_stream(dev).wait_stream(stream)
        self.sampler.counter.zero_()   # the warm-up draws do not count: step k uses draw index k
        if recorder is not None:
            recorder.restart()         # nor do the warm-up steps it recorded: the cursor starts at zero
        self.reset()

    def _body(self):
        r = self.runner
        rec = self.recorder
        if rec is not None:
            rec.begin()
        if self.chain:
            s = self.sampler
            r.step(self.flat, self.packed, self.S, self.frame_u8, self._ws, self.h, self.c, self._logits,
                   self._values, attn=self._attn, seed=s.seed, counter=s.counter, actions=self._actions,
                   logp=self._logp, core_h=self.core_h, core_c=self.core_c)
            if rec is not None:
                rec.record(self._actions, self._logp)
            return self._actions, self._logp, self._logits, self._values, self._attn
        X = self.frame_u8                  # uint8, cast in-kernel (AAA_FLAG_FRAMES_U8)
        ws = r.new_workspace()
        out = r.forward(self.flat, self.packed, self.S, X, ws, h0=self.h, c0=self.c, want_attn=True,
                        want_state=True, core=(self.core_h, self.core_c) if self.stateful else None)
        logits, values, attn, hT, cT = out[:5]
        action, logp = self.sampler(logits[0])
        self.h.copy_(hT)
        self.c.copy_(cT)
        if self.stateful:
            self.core_h.copy_(out[5])
            self.core_c.copy_(out[6])
        if rec is not None:
            rec.record(action, logp)
        return action, logp, logits[0], values[0], attn[0]

    def _refresh(self):
        key = tuple((p.data_ptr(), p._version) for p in self.params)
        if key != self._key:
            with torch.no_grad():
                torch.cat([p.detach().reshape(-1) for p in self.params], out=self.flat)
                self.runner.pack(self.flat, self.packed)
            self._key = key

    def reset(self):
        self.h.zero_()
        self.c.zero_()
        if self.stateful:
            self.core_h.zero_()
            self.core_c.zero_()
        if self.recorder is not None:   # the next step starts an episode in every row
            self.recorder.episode_start()

    @property
    def logits(self):
        return self._outs[2]

    @property
    def values(self):
        return self._outs[3]

    @property
    def log_prob(self):
        return self._outs[1]

    @property
    def attention(self):
        return self._outs[4]

    def step(self, observation, reward=None, done=None):
        """observation: uint8 (H, W, 3) / (B, H, W, 3) numpy array or tensor.

        With a recorder, ``reward`` and ``done`` (B,) are what the environment
        returned WITH this observation -- the result of the previous step's
        action; ``done[b] != 0`` says row b's observation is the first of a new
        episode.  None is zeros.  On the first step after ``reset()`` every row
        starts an episode whatever ``done`` says."""
        self._refresh()
        rec = self.recorder
        if rec is None and (reward is not None or done is not None):
            raise ValueError("GraphActor.step: reward / done belong to an actor with a recorder")
        if rec is not None and rec.fresh:
            done = None   # reset() / restart() have set done_in = 1
        on_dev = [isinstance(x, torch.Tensor) and x.is_cuda for x in (observation, reward, done)]
        ring = not on_dev[0] or (reward is not None and not on_dev[1]) or (done is not None and not on_dev[2])
        if ring:
            slot = self._slot
            buf, copied = self._host[slot]
            self._slot = (slot + 1) % len(self._host)
            copied.synchronize()   # the H2D copies that read this slot's buffers 4 steps ago have run
        if on_dev[0]:
            self.frame_u8.view(self.B, self.H, self.W, 3).copy_(observation.reshape(self.B, self.H, self.W, 3))
        else:
            src = torch.as_tensor(np.ascontiguousarray(observation)).reshape(self.B, self.H, self.W, 3)
            buf.copy_(src)
            self.frame_u8.view(self.B, self.H, self.W, 3).copy_(buf, non_blocking=True)
        if rec is not None:
            given = ((reward, rec.reward_in), (done, rec.done_in))
            if all(x is not None and not on_dev[1 + i] for i, (x, _) in enumerate(given)):
                stage, stage_np = self._host_rd[slot]   # both from the host, the usual case: one upload
                stage_np[0], stage_np[1] = np.asarray(reward).reshape(self.B), np.asarray(done).reshape(self.B)
                rec.rd_in.copy_(stage, non_blocking=True)
                rec.clear = [False, False]
                given = ()
            for i, (x, dst) in enumerate(given):
                if x is None:   # zeros: written once, then known to be there
                    if not rec.clear[i] and not (i == 1 and rec.fresh):
                        dst.zero_()
                        rec.clear[i] = True
                    continue
                rec.clear[i] = False
                if on_dev[1 + i]:
                    dst.copy_(x.reshape(self.B))
                else:
                    stage, stage_np = self._host_rd[slot]
                    stage_np[i] = np.asarray(x).reshape(self.B)
                    dst.copy_(stage[i], non_blocking=True)
            rec.fresh = False
        if ring:
            copied.record(torch.cuda.current_stream(self.device))
        self.graph.replay()
        if rec is not None:
            rec.steps += 1
        return self._outs[0]
