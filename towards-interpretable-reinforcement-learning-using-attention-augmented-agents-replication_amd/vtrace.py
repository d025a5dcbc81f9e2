"""V-trace actor-critic loss on the device.

The reference trains with REINFORCE on whole episodes as a stand-in
(main_mp.py:95); the paper it replicates trains with IMPALA: V-trace
actor-critic on fixed-length unrolls collected by actors that lag the
learner.  ``vtrace_loss`` computes that loss for B unrolls of T steps from
the unrolled logits and values, the actions taken, the rewards and the
behaviour log-probabilities the actors returned (``aaa_actor_step``'s
``logp``), in one kernel (csrc/loss.hip, C ABI ``aaa_vtrace``; include/aaa.h
has the definitions) that also writes d loss / d logits and d loss / d values,
so ``loss.backward()`` hands both cotangents straight to the hand-written
BPTT.  There is no CPU fallback.

``vtrace_cotangents`` is the bare launch into caller-owned buffers: no
validation that would read the device, no allocation it was not asked for, no
host sync -- what ``Learner.step_vtrace`` runs.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as N

__all__ = ["vtrace_loss", "vtrace_cotangents", "episode_starts", "HPARAMS"]

# the loss's scalars and their defaults (IMPALA's: clips at 1, baseline cost 0.5, entropy cost 0.01)
HPARAMS = dict(gamma=0.99, lam=1.0, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, baseline_cost=0.5,
               entropy_cost=0.01, scale=1.0, value_col=0)


def episode_starts(done, first=None):
    """The episode-start mask of an unroll cut out of longer episodes, (T, B)
    fp32 on ``done``'s device: row 0 is ``first`` (B; zeros when None: the
    unroll continues the state it is given) and row t is ``done[t - 1]`` -- the
    step after an episode's last one enters from ``reset()``.  What
    ``Agent.unroll(reset=)`` and ``Learner.step_vtrace(reset=)`` take
    (include/aaa.h ``aaa_forward_resets``).  Runs on the device; nothing is
    read back."""
    done = torch.as_tensor(done)
    if done.dim() != 2:
        raise ValueError(f"episode_starts: done must be (T, B), got {tuple(done.shape)}")
    out = torch.zeros(done.shape, dtype=torch.float32, device=done.device)
    if first is not None:
        out[0] = torch.as_tensor(first).to(device=done.device, dtype=torch.float32).reshape(-1)
    out[1:] = done[:-1].to(torch.float32)
    return out


def vtrace_cotangents(logits, values, actions, rewards, behaviour_logp, done, bootstrap, dlogits, dvalues,
                      vs=None, pg_adv=None, loss=None, *, steps=None, **hparams) -> None:
    """Enqueue ``aaa_vtrace`` on torch's current stream.  Every tensor is
    contiguous device memory of the layout include/aaa.h states (fp32; actions
    int32); ``behaviour_logp``, ``done``, ``bootstrap``, ``vs``, ``pg_adv`` and
    ``loss`` may be None.  ``steps`` runs the loss over the first ``steps``
    steps only (a contiguous prefix of the (T, B, A) layout).  Nothing here
    reads the device: an action outside [0, A) is not refused, it makes its
    row's outputs NaN."""
    hp = dict(HPARAMS)
    unknown = set(hparams) - set(hp)
    if unknown:
        raise TypeError(f"vtrace: unknown hyper-parameter(s) {sorted(unknown)}")
    hp.update(hparams)
    T, B, A = logits.shape
    T = T if steps is None else int(steps)
    d = N.VtraceDesc(T, B, A, int(hp["value_col"]), float(hp["gamma"]), float(hp["lam"]), float(hp["rho_bar"]),
                     float(hp["c_bar"]), float(hp["pg_rho_bar"]), float(hp["baseline_cost"]),
                     float(hp["entropy_cost"]), float(hp["scale"]))
    io = N.VtraceIO(*[N.ptr(t) for t in (logits, values, actions, rewards, behaviour_logp, done, bootstrap,
                                         dlogits, dvalues, vs, pg_adv, loss)])
    N.check(N.load().aaa_vtrace(ctypes.byref(d), ctypes.byref(io), N.stream_ptr(logits.device)), "vtrace")


class _VtraceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, values, actions, rewards, behaviour_logp, done, bootstrap, last, hp):
        T, B, A = logits.shape
        lg = logits.detach().contiguous()
        vl = values.detach().contiguous()
        dl, dv = torch.empty_like(lg), torch.empty_like(vl)
        n = T - 1 if last else T
        if last:   # the last step only supplies the bootstrap value; its cotangents are zero
            bootstrap = vl[T - 1, :, int(hp["value_col"])].contiguous()
            dl[n:].zero_()
            dv[n:].zero_()
        vs = torch.empty(n, B, device=lg.device, dtype=torch.float32)
        adv = torch.empty_like(vs)
        parts = torch.empty(B, 3, device=lg.device, dtype=torch.float32)
        vtrace_cotangents(lg, vl, actions, rewards, behaviour_logp, done, bootstrap, dl, dv, vs, adv, parts,
                          steps=n, **hp)
        ctx.save_for_backward(dl, dv)
        ctx.mark_non_differentiable(vs, adv, parts)
        total = float(hp["scale"]) * (parts[:, 0] + float(hp["baseline_cost"]) * parts[:, 1]
                                      - float(hp["entropy_cost"]) * parts[:, 2]).sum()
        return total, vs, adv, parts

    @staticmethod
    def backward(ctx, g_loss, g_vs, g_adv, g_parts):
        dl, dv = ctx.saved_tensors
        return (dl * g_loss, dv * g_loss) + (None,) * 7


def _tb(x, T, B, dev, dtype, name):
    if x is None:
        return None
    x = torch.as_tensor(x)
    if x.numel() != T * B:
        raise ValueError(f"{name} must be (T, B) = ({T}, {B}), got {tuple(x.shape)}")
    return x.reshape(T, B).to(device=dev, dtype=dtype).contiguous()


def vtrace_loss(logits: torch.Tensor, values: torch.Tensor, actions, rewards, behaviour_logp=None, done=None,
                bootstrap=None, *, gamma: float = 0.99, lam: float = 1.0, rho_bar: float = 1.0, c_bar: float = 1.0,
                pg_rho_bar: float = 1.0, baseline_cost: float = 0.5, entropy_cost: float = 0.01,
                scale: float = 1.0, value_col: int = 0, return_extras: bool = False):
    """V-trace actor-critic loss of B unrolls of T steps (include/aaa.h ``aaa_vtrace``):

        scale * sum_{t,b} [ -adv_t log pi_t[a_t] + baseline_cost (vs_t - V_t)^2 / 2 - entropy_cost H_t ]

    logits, values (T, B, A) fp32 on the gfx950 device (e.g. from
    ``Agent.unroll``); the baseline is ``values[..., value_col]``.  actions
    (T, B) ints in [0, A), rewards (T, B), behaviour_logp (T, B) the log-prob
    of each action under the policy that drew it (None: on-policy), done
    (T, B) non-zero where the episode ended with that step's transition (it
    cuts the return only: the unroll's recurrent state is carried across it),
    bootstrap (B) the value after the last step (None: 0).
    ``bootstrap="last"`` is the IMPALA convention: the unroll's last step only
    supplies the bootstrap value, the loss runs over steps 0..T-2 (the other
    (T, B) inputs may have T or T-1 steps) and the last step's cotangents are
    zero.  vs and the advantages are constants of the differentiation;
    ``.backward()`` puts the kernel's dlogits / dvalues on ``logits`` /
    ``values``.  Returns the scalar loss, and with ``return_extras`` also
    ``(vs, pg_adv, loss_parts)``: (T, B), (T, B) -- T-1 steps with
    ``bootstrap="last"`` -- and the raw per-row sums (B, 3)
    ``[-adv log pi[a], (vs - V)^2 / 2, H]``.
    """
    if logits.dim() != 3:
        raise ValueError(f"logits must be (T, B, A), got {tuple(logits.shape)}")
    if values.shape != logits.shape:
        raise ValueError(f"values must have logits' shape {tuple(logits.shape)}, got {tuple(values.shape)}")
    for name, x in (("logits", logits), ("values", values)):
        if not x.is_cuda or x.dtype != torch.float32:
            raise RuntimeError(f"vtrace_loss: {name} must be fp32 on the gfx950 device (there is no CPU fallback)")
    if values.device != logits.device:
        raise RuntimeError("vtrace_loss: logits and values must be on one device")
    T, B, A = logits.shape
    if A < 2:
        raise ValueError(f"vtrace_loss: need at least 2 actions, got A = {A}")
    if not 0 <= int(value_col) < A:
        raise ValueError(f"value_col must lie in [0, {A})")
    last = isinstance(bootstrap, str)
    if last and bootstrap != "last":
        raise ValueError(f"bootstrap must be a (B) tensor, None or \"last\", got {bootstrap!r}")
    n = T - 1 if last else T
    if n < 1:
        raise ValueError("bootstrap=\"last\" needs an unroll of at least 2 steps")
    dev = logits.device

    def steps(x, dtype, name):
        if x is not None and last and torch.as_tensor(x).numel() == T * B:
            x = torch.as_tensor(x).reshape(T, B)[:n]
        return _tb(x, n, B, dev, dtype, name)

    actions = torch.as_tensor(actions)
    if actions.numel() and (int(actions.min()) < 0 or int(actions.max()) >= A):
        raise ValueError(f"actions must lie in [0, {A})")
    actions = steps(actions, torch.int32, "actions")
    rewards = steps(rewards, torch.float32, "rewards")
    behaviour_logp = steps(behaviour_logp, torch.float32, "behaviour_logp")
    done = steps(done, torch.float32, "done")
    if not last and bootstrap is not None:
        bootstrap = torch.as_tensor(bootstrap)
        if bootstrap.numel() != B:
            raise ValueError(f"bootstrap must be (B) = ({B}), got {tuple(bootstrap.shape)}")
        bootstrap = bootstrap.detach().reshape(B).to(device=dev, dtype=torch.float32).contiguous()
    hp = dict(gamma=gamma, lam=lam, rho_bar=rho_bar, c_bar=c_bar, pg_rho_bar=pg_rho_bar,
              baseline_cost=baseline_cost, entropy_cost=entropy_cost, scale=scale, value_col=value_col)
    loss, vs, adv, parts = _VtraceFn.apply(logits, values, actions, rewards, behaviour_logp, done,
                                           None if last else bootstrap, last, hp)
    return (loss, vs, adv, parts) if return_extras else loss
