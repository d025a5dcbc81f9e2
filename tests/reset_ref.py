"""Reference for episode starts inside an unroll (include/aaa.h
``aaa_forward_resets``): ``oracle.ref_cpu.unroll`` composed step by step, the
state of a row with ``reset[t][b] != 0`` replaced by the ``reset()`` state
(zeros, attention.py:142-149) before step t -- what the reference does when it
calls ``agent.reset()`` at an episode start (main_mp.py:100), for that row
alone.  The replacement is ``torch.where``, a select: autograd then gives the
cut gradient, and nothing of the state before a reset (NaN included) reaches
anything after it.  The oracle itself is not edited.
"""
import torch

from oracle import ref_cpu


def _select(keep, s):
    """s with the rows where ``keep`` is False replaced by zeros ((B, ...) tensors)."""
    k = keep.view(-1, *([1] * (s.dim() - 1)))
    return torch.where(k, s, torch.zeros_like(s))


def unroll(P, X, reset, state=None, core_state=None, stateful_core=False, **kw):
    """X (T, B, H, W, 3), reset (T, B) -> logits, values, attn stacked over T and
    the final state as ``ref_cpu.unroll(..., return_state=True)`` returns it.
    ``state`` = (h, c) in the oracle's (B, 128, w, h) layout, ``core_state`` =
    (h, c) (B, 256); None = the reset() state."""
    T = X.shape[0]
    pr, pa = kw.pop("prev_reward", None), kw.pop("prev_action", None)
    L, V, A = [], [], []
    for t in range(T):
        keep = reset[t] == 0
        if state is not None:
            state = tuple(_select(keep, s) for s in state)
        if core_state is not None:
            core_state = tuple(_select(keep, s) for s in core_state)
        lg, vl, at, st = ref_cpu.unroll(P, X[t:t + 1], state=state, core_state=core_state,
                                        stateful_core=stateful_core, return_state=True,
                                        prev_reward=None if pr is None else pr[t:t + 1],
                                        prev_action=None if pa is None else pa[t:t + 1], **kw)
        state, core_state = st if stateful_core else (st, None)
        L.append(lg[0]), V.append(vl[0]), A.append(at[0])
    final = (state, core_state) if stateful_core else state
    return torch.stack(L), torch.stack(V), torch.stack(A), final


def grads(P):
    return {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in P.items()}
