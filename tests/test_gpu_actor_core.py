"""The stateful policy core on the small-batch actor chain
(aaa_actor_step_core; attention.py:324-331, 356-358): the chain against the
learner's T=1 stateful forward on the same carried states, its out-of-place
state outputs, and GraphActor over a stateful agent against the oracle's
stateful unroll -- on the chain and on the learner's forward.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_close, detinit
from oracle import ref_cpu

import attention
from aaa_amd.policy import sample_actions

pytestmark = pytest.mark.gpu

A = 18


def _setup(cuda, H, W, B, nq, u8, seed=3):
    from aaa_amd.runtime import ActorRunner
    params = detinit.deterministic_params(seed, A, nq)
    ar = ActorRunner(B, H, W, nq, A, cuda, frames_u8=u8, stateful_core=True)
    agent = attention.Agent(A, num_queries=nq, grid=(ar.h, ar.w), stateful_core=True)
    detinit.load_into(agent, params)
    flat = torch.cat([p.detach().reshape(-1) for p in agent.parameters()]).to(cuda)
    assert flat.numel() == ar.n_params
    packed = ar.new_packed()
    ar.pack(flat, packed)
    S = agent.spatial.S.to(cuda).contiguous()
    return params, ar, flat, packed, S


def _states(ar, B, g, cuda):
    h = (torch.rand(ar.state_shape(), generator=g) * 2 - 1).to(cuda) * 0.5
    c = (torch.rand(ar.state_shape(), generator=g) * 2 - 1).to(cuda)
    core_h = ((torch.rand(B, 256, generator=g) * 2 - 1) * 0.5).to(cuda)   # uniform in +-0.5, per row
    core_c = (torch.rand(B, 256, generator=g) * 2 - 1).to(cuda)           # uniform in +-1
    return h, c, core_h, core_c


def _query_ref(params, core_h, nq):
    """QueryNetwork (attention.py:184-198) with torch on the CPU, in float64."""
    x = core_h.detach().cpu().double()
    for i, relu in ((0, True), (2, True), (4, False)):
        w = torch.from_numpy(params[f"query.model.{i}.weight"]).double()
        b = torch.from_numpy(params[f"query.model.{i}.bias"]).double()
        x = torch.nn.functional.linear(x, w, b)
        if relu:
            x = x.clamp_min(0)
    return x.reshape(-1, nq, 72).numpy()


@pytest.mark.parametrize("H,W,B,nq,u8", [(84, 84, 1, 4, True), (84, 84, 3, 8, False), (210, 160, 2, 4, True),
                                         (84, 84, 16, 4, True)])
def test_actor_core_chain_matches_learner_forward(cuda, H, W, B, nq, u8):
    """aaa_actor_step_core against aaa_forward with AAA_FLAG_STATEFUL_CORE and
    T=1 on the same ConvLSTM state, core state, prev_reward / prev_action,
    frames and packed weights: logits, values, attention, h, c, core_h, core_c
    at 1e-4 over three chained steps (continuing from the learner's states); the
    fused draw bit-identical to aaa_sample_actions on the chain's own logits;
    and the ``query`` output against the three-layer MLP evaluated on the CPU,
    at 1e-5 of its largest element, with rows that really differ."""
    from aaa_amd.runtime import UnrollRunner
    params, ar, flat, packed, S = _setup(cuda, H, W, B, nq, u8)
    ur = UnrollRunner(B, 1, H, W, nq, A, "fp32", cuda, stateful_core=True, frames_u8=u8)
    g = torch.Generator().manual_seed(H + B + nq)
    h, c, core_h, core_c = _states(ar, B, g, cuda)
    ws, uws = ar.new_workspace(), ur.new_workspace()
    counter = torch.tensor([5], dtype=torch.int64, device=cuda)
    for step in range(3):
        fr = torch.from_numpy(detinit.frames_u8(40 + step, (B, H, W, 3))).to(cuda)
        if not u8:
            fr = fr.float() * 0.5
        pr = torch.rand(B, generator=g).to(cuda)
        pa = torch.randint(0, A, (B,), generator=g).float().to(cuda)
        rl, rv, ra, rh, rc, rch, rcc = ur.forward(flat, packed, S, fr.unsqueeze(0), uws, prev_reward=pr,
                                                  prev_action=pa, h0=h, c0=c, want_attn=True, want_state=True,
                                                  core=(core_h, core_c))
        qref = _query_ref(params, core_h, nq)
        logits = torch.empty(B, A, device=cuda)
        values = torch.empty(B, A, device=cuda)
        attn = torch.empty(B, ar.h, ar.w, nq, device=cuda)
        acts = torch.empty(B, dtype=torch.int32, device=cuda)
        logp = torch.empty(B, device=cuda)
        query = torch.empty(B, nq, 72, device=cuda)
        c_before = counter.clone()
        ar.step(flat, packed, S, fr, ws, h, c, logits, values, attn=attn, prev_reward=pr, prev_action=pa,
                seed=77, counter=counter, actions=acts, logp=logp, core_h=core_h, core_c=core_c, query=query)
        torch.cuda.synchronize()
        for name, got, ref in (("logits", logits, rl[0]), ("values", values, rv[0]), ("attention", attn, ra[0]),
                               ("h", h, rh), ("c", c, rc), ("core_h", core_h, rch), ("core_c", core_c, rcc)):
            assert_close(got.cpu().numpy(), ref.cpu().numpy(), 1e-4, f"{name} step {step}")
        assert int(counter.item()) == int(c_before.item()) + 1
        sa, slp = sample_actions(logits, seed=77, counter=c_before)
        assert torch.equal(sa, acts) and torch.equal(slp, logp)
        qbound = 1e-5 * float(np.abs(qref).max())
        qerr = float(np.abs(query.cpu().numpy().astype(np.float64) - qref).max())
        assert qerr <= qbound, (step, qerr, qbound)
        if B > 1:   # the rows' queries really differ: a shared query would not pass the per-row check
            assert float(np.abs(qref[0] - qref[1]).max()) > 100 * qbound
        # continue from the learner's states so both paths see the same inputs next step
        for dst, src in ((h, rh), (c, rc), (core_h, rch), (core_c, rcc)):
            dst.copy_(src)


@pytest.mark.parametrize("B,nq", [(1, 4), (3, 8)])
def test_actor_core_out_of_place_equals_in_place(cuda, B, nq):
    """The same step with core_h_out / core_c_out: bit-identical outputs, and
    core_h / core_c are then only read."""
    H = W = 84
    params, ar, flat, packed, S = _setup(cuda, H, W, B, nq, True)
    g = torch.Generator().manual_seed(11 + B)
    h0, c0, ch0, cc0 = _states(ar, B, g, cuda)
    fr = torch.from_numpy(detinit.frames_u8(7, (B, H, W, 3))).to(cuda)
    ws = ar.new_workspace()
    res = []
    for oop in (False, True):
        h, c, ch, cc = h0.clone(), c0.clone(), ch0.clone(), cc0.clone()
        out = [torch.empty(B, A, device=cuda), torch.empty(B, A, device=cuda),
               torch.empty(B, ar.h, ar.w, nq, device=cuda), torch.empty(B, nq, 72, device=cuda)]
        cho = torch.full((B, 256), 7.0, device=cuda) if oop else None
        cco = torch.full((B, 256), 7.0, device=cuda) if oop else None
        ar.step(flat, packed, S, fr, ws, h, c, out[0], out[1], attn=out[2], core_h=ch, core_c=cc,
                core_h_out=cho, core_c_out=cco, query=out[3])
        torch.cuda.synchronize()
        if oop:
            assert torch.equal(ch, ch0) and torch.equal(cc, cc0)
        res.append(out + [h, c, cho if oop else ch, cco if oop else cc])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][6], ch0) and not torch.equal(res[0][7], cc0)


@functools.lru_cache(maxsize=None)
def _oracle_episode():
    """detinit params seed 0, five steps of two rows at 84x84: the oracle's
    stateful unroll, and its zero-state unroll to tell the two apart."""
    params = detinit.deterministic_params(0, A, 4)
    frames = detinit.frames_u8(31, (5, 2, 84, 84, 3))
    P = ref_cpu.tensor_params(params, requires_grad=False)
    X = torch.from_numpy(frames.astype(np.float32))
    with torch.no_grad():
        rl, _, ra = ref_cpu.unroll(P, X, stateful_core=True)
        zl, _, _ = ref_cpu.unroll(P, X)
    return params, frames, rl.numpy(), ra.numpy(), zl.numpy()


@pytest.mark.parametrize("chain", [True, False])
def test_graph_actor_stateful_matches_oracle(cuda, chain):
    """GraphActor over a stateful agent -- on the actor chain or the learner's
    T=1 forward -- is the oracle's stateful agent step by step: logits at 1e-4,
    every draw, the last attention map; reset() restarts the episode bit for
    bit; an in-place parameter update is re-packed.  The oracle's zero-state
    logits differ from its stateful ones by far more than the tolerance from
    step 1 on, so a zero-state replay cannot pass."""
    from aaa_amd.policy import GraphActor
    params, frames, rl, ra, zl = _oracle_episode()
    T, B = frames.shape[:2]
    for t in range(1, T):
        assert float(np.abs(rl[t] - zl[t]).max()) > 1e-3, t
    agent = attention.Agent(A, grid=(11, 11), stateful_core=True)
    detinit.load_into(agent, params)
    agent.to(cuda)
    ga = GraphActor(agent, 84, 84, B=B, seed=9, chain=chain)
    assert ga.chain == chain
    ga.reset()
    got_a, got_l = [], []
    for t in range(T):
        a = ga.step(frames[t])
        got_a.append(a.cpu().numpy().copy())
        got_l.append(ga.logits.clone())
    attn = ga.attention.cpu().numpy()
    for t in range(T):
        assert_close(got_l[t].cpu().numpy(), rl[t], 1e-4, f"logits t={t}")
        oa, _, margin = ref_cpu.sample_actions(rl[t], 9, t)
        assert float(margin.min()) > 1e-4, (t, margin)   # every draw counts: none is near a CDF boundary
        assert np.array_equal(got_a[t], oa), t
    assert_close(attn, ra[T - 1], 1e-4, "attention")
    # reset() zeroes the ConvLSTM and the core state: step 0 again, bit for bit
    ga.reset()
    ga.step(frames[0])
    assert torch.equal(ga.logits, got_l[0])
    with torch.no_grad():
        agent.policy_head[0].bias.add_(1.0)
    ga.reset()
    ga.step(frames[0])
    assert_close(ga.logits.cpu().numpy(), rl[0] + 1.0, 1e-4, "logits after bias update")


def test_graph_actor_picks_the_chain_for_stateful_agents(cuda):
    """chain=None: fp32 stateful agents with B <= 16 act on the chain; the
    zero-state agent still does."""
    from aaa_amd.policy import GraphActor
    params = detinit.deterministic_params(0, A, 4)
    for stateful in (True, False):
        agent = attention.Agent(A, grid=(11, 11), stateful_core=stateful)
        detinit.load_into(agent, params)
        agent.to(cuda)
        ga = GraphActor(agent, 84, 84, B=1, seed=1)
        assert ga.chain is True
        assert (ga.core_h is not None) == stateful
