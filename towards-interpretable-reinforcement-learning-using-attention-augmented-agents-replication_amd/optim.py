"""Drop-in fused Adam for the learner.

The reference trains with ``optim.Adam(policy.parameters(), lr=1e-3)``
(main_mp.py:92) and calls ``optimizer.step()`` after every episode's backward
(main_mp.py:78).  ``aaa_amd.optim.Adam`` takes the same constructor arguments
and keeps the same per-parameter state (``step``, ``exp_avg``,
``exp_avg_sq`` [, ``max_exp_avg_sq``]) so a torch.optim.Adam state_dict loads
into it and back; ``step()`` is ONE fused multi-tensor HIP launch
(csrc/optim.hip, C ABI ``aaa_adam_step``) instead of torch's seven foreach
passes.  There is no CPU fallback: parameters must be fp32 tensors on the
gfx950 device.

``aaa_amd.optim.RMSprop`` / ``rmsprop_flat_`` are the same for
``torch.optim.RMSprop`` (C ABI ``aaa_rmsprop_step``), the optimizer IMPALA
trains with, with TensorFlow's placement of eps and a linear learning-rate
anneal on the device as extensions.
"""
from __future__ import annotations

from collections import defaultdict

import torch
from torch.autograd.graph import increment_version

from . import _native as N

__all__ = ["Adam", "adam_flat_", "clip_grad_norm_", "RMSprop", "rmsprop_flat_", "rmsprop_lr"]


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 maximize: bool = False, foreach=None, capturable: bool = False, differentiable: bool = False,
                 fused=None):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if differentiable:
            raise RuntimeError("aaa_amd.optim.Adam: differentiable=True is not supported by the fused kernel")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused)
        super().__init__(params, defaults)

    @staticmethod
    def _hp(group) -> N.AdamHP:
        b1, b2 = group["betas"]
        return N.AdamHP(float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                        float(group["weight_decay"]), 1 if group["amsgrad"] else 0, 1 if group["maximize"] else 0)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _step_groups(self, "Adam", N.adam_step, lambda group: (
            ("exp_avg", True), ("exp_avg_sq", True), ("max_exp_avg_sq", bool(group["amsgrad"]))))
        return loss


class RMSprop(torch.optim.Optimizer):
    """Drop-in fused ``torch.optim.RMSprop`` (include/aaa.h ``aaa_rmsprop_step``): the same
    constructor arguments, validation and per-parameter state (``step``, ``square_avg``, and
    ``momentum_buffer`` / ``grad_avg`` only when used), so a torch state_dict loads into it and
    back; ``step()`` is one fused launch per 48 tensors.  Keyword-only extensions:
    ``eps_in_sqrt`` (TensorFlow's sqrt(v + eps), as IMPALA uses it, instead of torch's
    sqrt(v) + eps) and a linear anneal of the learning rate from ``lr`` to ``lr_end`` over
    ``anneal_steps`` updates (0: constant).  With momentum the buffer is torch's, the learning
    rate outside it.  There is no CPU fallback."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False,
                 capturable=False, foreach=None, maximize=False, differentiable=False, *,
                 eps_in_sqrt: bool = False, lr_end: float = 0.0, anneal_steps: int = 0):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= momentum:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0.0 <= alpha:
            raise ValueError(f"Invalid alpha value: {alpha}")
        if not 0.0 <= lr_end:
            raise ValueError(f"Invalid lr_end value: {lr_end}")
        if int(anneal_steps) != anneal_steps or anneal_steps < 0:
            raise ValueError(f"Invalid anneal_steps value: {anneal_steps}")
        if differentiable:
            raise RuntimeError("aaa_amd.optim.RMSprop: differentiable=True is not supported by the fused kernel")
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay,
                        capturable=capturable, foreach=foreach, maximize=maximize, differentiable=differentiable,
                        eps_in_sqrt=eps_in_sqrt, lr_end=lr_end, anneal_steps=int(anneal_steps))
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:   # a torch.optim.RMSprop state_dict has no extension keys
            group.setdefault("eps_in_sqrt", False)
            group.setdefault("lr_end", 0.0)
            group.setdefault("anneal_steps", 0)
            for p in group["params"]:
                st = self.state.get(p, {})
                if len(st) != 0 and not torch.is_tensor(st["step"]):
                    st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)

    @staticmethod
    def _hp(group) -> N.RmspropHP:
        return _rmsprop_hp(**{k: group[k] for k in ("lr", "alpha", "eps", "weight_decay", "momentum", "centered",
                                                     "maximize", "eps_in_sqrt", "lr_end", "anneal_steps")})

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _step_groups(self, "RMSprop", N.rmsprop_step, lambda group: (
            ("square_avg", True), ("momentum_buffer", group["momentum"] > 0), ("grad_avg", bool(group["centered"]))))
        return loss


def _step_groups(opt, name, launch, state_keys) -> None:
    """The per-group loop of ``Adam.step`` / ``RMSprop.step``.  ``state_keys(group)``: the
    (state key, wanted?) pairs of the group's buffers, in the order ``launch`` -- ``_native``'s
    adam_step / rmsprop_step -- takes them after (hp, step, params, grads); a buffer not wanted
    is never created and goes in as None.  One launch per distinct step value."""
    for group in opt.param_groups:
        keys = state_keys(group)
        by_step = defaultdict(lambda: tuple([] for _ in range(2 + len(keys))))
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.grad.is_sparse:
                raise RuntimeError(f"{name} does not support sparse gradients")
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"aaa_amd.optim.{name}: parameters must be contiguous fp32 tensors on the "
                                   "gfx950 device (there is no CPU fallback)")
            st = opt.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                for key, wanted in keys:
                    if wanted:
                        st[key] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            lists = by_step[int(st["step"].item())]
            lists[0].append(p)
            lists[1].append(p.grad.contiguous())
            for lst, (key, wanted) in zip(lists[2:], keys):
                if wanted:
                    lst.append(st[key])
        hp = opt._hp(group)
        for step, (ps, gs, *states) in by_step.items():
            launch(hp, step, ps, gs, *[lst if wanted else None for lst, (_, wanted) in zip(states, keys)],
                   stream=N.stream_ptr(ps[0].device))
            _bump_versions(ps)


def _rmsprop_hp(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, maximize=False,
                eps_in_sqrt=False, lr_end=0.0, anneal_steps=0) -> N.RmspropHP:
    return N.RmspropHP(float(lr), float(alpha), float(eps), float(weight_decay), float(momentum), float(lr_end),
                       int(anneal_steps), 1 if centered else 0, 1 if maximize else 0, 1 if eps_in_sqrt else 0)


def rmsprop_lr(n: int, lr: float, lr_end: float = 0.0, anneal_steps: int = 0) -> float:
    """The learning rate of the update after ``n`` applied ones (include/aaa.h aaa_rmsprop_step):
    lr_end + (lr - lr_end) * max(0, 1 - n / anneal_steps) in double; anneal_steps = 0 is a constant lr."""
    if anneal_steps <= 0:
        return float(lr)
    return float(lr_end) + (float(lr) - float(lr_end)) * max(0.0, 1.0 - n / anneal_steps)


def rmsprop_flat_(params: torch.Tensor, grads: torch.Tensor, square_avg: torch.Tensor, step: int, *,
                  momentum_buf: torch.Tensor | None = None, grad_avg: torch.Tensor | None = None,
                  guard: torch.Tensor | None = None, step_dev: torch.Tensor | None = None,
                  clip: torch.Tensor | None = None, **hparams) -> None:
    """RMSProp over one flat fp32 buffer (the Learner's state_dict-ordered params): one launch.
    ``hparams``: lr, alpha, eps, weight_decay, momentum, centered, maximize, eps_in_sqrt, lr_end,
    anneal_steps (torch.optim.RMSprop's defaults; the last three as aaa_amd.optim.RMSprop).
    ``momentum_buf`` is needed iff momentum > 0, ``grad_avg`` iff centered.  ``guard``,
    ``step_dev`` and ``clip`` as for adam_flat_ (here ``clip`` does not need ``step_dev``); with
    ``step_dev`` the anneal follows the updates applied on the device, otherwise ``step`` - 1."""
    hp = _rmsprop_hp(**hparams)
    N.rmsprop_step(hp, step, [params], [grads], [square_avg], None if momentum_buf is None else [momentum_buf],
                   None if grad_avg is None else [grad_avg], stream=N.stream_ptr(params.device), guard=guard,
                   step_dev=step_dev, clip=clip)
    _bump_versions([params])


def _bump_versions(ps) -> None:
    """The kernel writes the parameters through raw pointers, which autograd's
    version counters do not see; bump them as an in-place torch op would, so
    every cache keyed on (data_ptr, _version) -- Agent's packed weights,
    GraphActor's re-pack check -- sees the update (and autograd still catches
    a stale saved parameter)."""
    for p in ps:
        increment_version(p)


def adam_flat_(params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               step: int, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
               guard: torch.Tensor | None = None, step_dev: torch.Tensor | None = None,
               clip: torch.Tensor | None = None) -> None:
    """Adam over one flat fp32 buffer (the Learner's state_dict-ordered params): one launch.
    ``guard`` (one fp32 device element): skip the update on the device when it is non-zero.
    ``step_dev`` (one int32 device element, updates applied so far): use it instead of
    ``step`` and advance it on the device only when the update ran.
    ``clip`` (the 4-element stats ``_native.grad_norm`` wrote; needs ``step_dev``): the update
    runs on ``grads * clip[1]`` and is skipped, like a guarded one, when ``clip[2] != 0``."""
    hp = N.AdamHP(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), 0, 0)
    N.adam_step(hp, step, [params], [grads], [exp_avg], [exp_avg_sq], None, stream=N.stream_ptr(params.device),
                guard=guard, step_dev=step_dev, clip=clip)
    _bump_versions([params])


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, *,
                    stats: torch.Tensor | None = None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` on the device (include/aaa.h ``aaa_grad_norm`` +
    ``aaa_grad_scale``): the total 2-norm of the parameters' gradients, summed in
    double in a fixed order, and the in-place scale by min(1, max_norm / (norm +
    1e-6)) -- over any number of contiguous fp32 device gradients, with no host
    sync.  Returns the 0-d device norm (element 0 of the stats; pass ``stats``, 4
    fp32 device elements, to keep [norm, coefficient, non-finite flag, max_norm]).
    ``error_if_nonfinite=True`` reads the flag, which syncs.  ``foreach`` is
    accepted and ignored.  There is no CPU fallback.

    ``stats=`` is an extension of torch's signature (keyword-only, so positional
    callers are unaffected): torch returns only the norm, and the coefficient and
    the flag would otherwise need a host read to recompute.  The scratch of the
    partial sums is allocated per call; torch's caching allocator hands a freed
    block to later work on the same stream only, so releasing it on return while
    the kernels are still queued is safe."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise ValueError(f"aaa_amd.optim.clip_grad_norm_: only norm_type=2 is supported (got {norm_type})")
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    for g in grads:
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
            raise RuntimeError("aaa_amd.optim.clip_grad_norm_: gradients must be contiguous fp32 tensors on the "
                               "gfx950 device (there is no CPU fallback)")
    dev = grads[0].device
    if stats is None:
        stats = torch.empty(4, device=dev)
    scratch = torch.empty(N.grad_norm_scratch_bytes([g.numel() for g in grads]) // 8, dtype=torch.float64, device=dev)
    st = N.stream_ptr(dev)
    N.grad_norm(float(max_norm), grads, stats, scratch, stream=st)
    if error_if_nonfinite and float(stats[2].item()) != 0.0:   # as torch: raised before any gradient is scaled
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is "
                           "non-finite, so it cannot be clipped. To disable this error and scale the gradients "
                           "by the non-finite norm anyway, set `error_if_nonfinite=False`")
    N.grad_scale(stats, grads, stream=st)
    for g in grads:
        increment_version(g)
    return stats[0]
