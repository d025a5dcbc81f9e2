"""The actor's unroll recorder on the device (aaa_unroll_begin / aaa_unroll_record,
csrc/unroll.hip): the kernels bit for bit against their numpy restatement
(tests/unroll_ref.py), GraphActor with a recorder in its captured step, and a
learner unroll that starts from the state the actor recorded."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import assert_close, detinit
from unroll_ref import UnrollRef, new_bank

import attention
from aaa_amd import _native as N

pytestmark = pytest.mark.gpu

A = 18
SENT_U8, SENT_I32, SENT_F32 = 0xA5, -77, -123.5


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _same(got, ref, what):
    """Bit-identical, NaN payloads and signed zeros included."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.flatnonzero(_bits(got) != _bits(ref))
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at byte {int(bad[0])}"


# ------------------------------------------------------------ kernel level --
@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("core", [0, 256])
@pytest.mark.parametrize("fb", [48, 75, 4800])
def test_kernels_match_the_restatement(cuda, fb, core, clip):
    """B = 3 rows at b0 = 1 of Bu = 5, T = 3, 2T + 1 steps: frame rows of three 16-byte
    vectors, of 75 bytes (the byte path, unaligned rows) and of 300 vectors (more than one
    pass of a workgroup).  An episode end on row 1 at every t = T-1 (both banks) with
    NaN planted in that row's state before it, rewards of +-3 with and without the clip.
    Every bank was prefilled with a sentinel: after every step the banks, the cursor and the
    live state equal the restatement's bit for bit, so rows 0 and 4 and every slot not yet
    reached still hold it."""
    T, B, Bu, b0, sf = 3, 3, 5, 1, 8
    rng = np.random.default_rng(fb + core + int(clip))
    banks = [new_bank(T, Bu, fb, sf, core, SENT_U8, SENT_I32, SENT_F32) for _ in (0, 1)]
    ref = UnrollRef(T, B, Bu, b0, fb, sf, core, clip, banks)
    dbanks = [{k: torch.from_numpy(v.copy()).to(cuda) for k, v in b.items()} for b in banks]
    live = dict(h=rng.standard_normal((B, sf)).astype(np.float32), c=rng.standard_normal((B, sf)).astype(np.float32))
    if core:
        live.update(core_h=rng.standard_normal((B, core)).astype(np.float32),
                    core_c=rng.standard_normal((B, core)).astype(np.float32))
    dlive = {k: torch.from_numpy(v.copy()).to(cuda) for k, v in live.items()}
    pos = torch.zeros(4, dtype=torch.int32, device=cuda)
    frame = torch.zeros(B, fb, dtype=torch.uint8, device=cuda)
    actions = torch.zeros(B, dtype=torch.int32, device=cuda)
    logp, reward_in, done_in = (torch.zeros(B, device=cuda) for _ in range(3))
    desc = N.UnrollDesc(T, B, Bu, b0, fb, sf, core, clip)
    io = N.UnrollIO()
    for k in (0, 1):
        for name in N.UNROLL_BANK_FIELDS:
            setattr(io.bank[k], name, N.ptr(dbanks[k].get(name)))
    for name, t in dict(pos=pos, frame=frame, actions=actions, logp=logp, reward_in=reward_in, done_in=done_in,
                        **{k: dlive.get(k) for k in ("h", "c", "core_h", "core_c")}).items():
        setattr(io, name, N.ptr(t))
    assert fb % 16 or all(io.bank[k].frames % 16 == 0 for k in (0, 1))
    st = N.stream_ptr(cuda)
    for s in range(2 * T + 1):
        t_slot = s if s < T else (s - 1) % (T - 1) + 1
        done = np.zeros(B, np.float32)
        if s == 0:
            done[:] = 1.0
        if s > 0 and t_slot == T - 1:
            done[1] = 2.0 if s == T - 1 else 1.0           # any non-zero value counts, and is stored as 1
            for v in live.values():
                v[1] = np.nan                              # must be zero after begin
        for k, v in live.items():
            dlive[k].copy_(torch.from_numpy(v))
        rew = (3.0 * (-1.0) ** (s + np.arange(B))).astype(np.float32)
        if s == 1:
            rew[2] = np.nan                                # stays NaN through the clip
        done_in.copy_(torch.from_numpy(done))
        reward_in.copy_(torch.from_numpy(rew))
        N.unroll_begin(desc, io, st)
        ref.begin(done, live["h"], live["c"], live.get("core_h"), live.get("core_c"))
        for k, v in live.items():
            _same(dlive[k], v, f"step {s}: {k} after begin")
        if done[1]:
            assert not live["h"][1].any() and not np.isnan(dlive["h"].cpu().numpy()[1]).any()
        for v in live.values():                             # the actor's step moves the state
            v += rng.standard_normal(v.shape).astype(np.float32)
        fr = rng.integers(0, 256, (B, fb), dtype=np.uint8)
        ac = rng.integers(0, A, B).astype(np.int32)
        lp = (-rng.random(B)).astype(np.float32)
        frame.copy_(torch.from_numpy(fr))
        actions.copy_(torch.from_numpy(ac))
        logp.copy_(torch.from_numpy(lp))
        N.unroll_record(desc, io, st)
        ref.record(fr, ac, lp, rew, done)
        _same(pos, ref.pos, f"step {s}: pos")
        for k in (0, 1):
            for name, v in banks[k].items():
                _same(dbanks[k][name], v, f"step {s}: bank {k} {name}")
    assert list(ref.pos) == [1, 1, 3, 0]                    # 2T + 1 = 7 steps at T = 3: three unrolls
    for k in (0, 1):                                        # spelled out: rows of other actors hold the sentinel
        assert (dbanks[k]["frames"][:, [0, 4]] == SENT_U8).all() and (dbanks[k]["h0"][[0, 4]] == SENT_F32).all()
        assert (dbanks[k]["actions"][:, [0, 4]] == SENT_I32).all() and (dbanks[k]["first"][[0, 4]] == SENT_F32).all()
    if clip:
        assert float(dbanks[1]["rewards"][:T - 1, b0:b0 + B].abs().max()) == 1.0
    else:
        assert float(dbanks[1]["rewards"][:T - 1, b0:b0 + B].abs().max()) == 3.0


def test_cursor_out_of_range_writes_nothing(cuda):
    """A cursor that is not a position (t >= T, a bank that is not 0 or 1) makes both calls no-ops."""
    T, B, Bu, fb, sf = 3, 2, 2, 48, 8
    banks = [{k: torch.from_numpy(v).to(cuda) for k, v in new_bank(T, Bu, fb, sf, 0, SENT_U8, SENT_I32, SENT_F32).items()}
             for _ in (0, 1)]
    before = [{k: v.clone() for k, v in b.items()} for b in banks]
    h, c = torch.ones(B, sf, device=cuda), torch.ones(B, sf, device=cuda)
    frame = torch.zeros(B, fb, dtype=torch.uint8, device=cuda)
    actions = torch.zeros(B, dtype=torch.int32, device=cuda)
    logp, reward_in, done_in = torch.zeros(B, device=cuda), torch.zeros(B, device=cuda), torch.ones(B, device=cuda)
    desc = N.UnrollDesc(T, B, Bu, 0, fb, sf, 0, 0.0)
    for bad in ([T, 0, 0, 0], [-1, 0, 0, 0], [0, 2, 0, 0], [1, -1, 5, 0]):
        pos = torch.tensor(bad, dtype=torch.int32, device=cuda)
        io = N.UnrollIO()
        for k in (0, 1):
            for name in N.UNROLL_BANK_FIELDS:
                setattr(io.bank[k], name, N.ptr(banks[k].get(name)))
        for name, t in dict(pos=pos, frame=frame, actions=actions, logp=logp, reward_in=reward_in, done_in=done_in,
                            h=h, c=c).items():
            setattr(io, name, N.ptr(t))
        N.unroll_begin(desc, io, N.stream_ptr(cuda))
        N.unroll_record(desc, io, N.stream_ptr(cuda))
        assert pos.tolist() == bad and bool((h == 1).all()) and bool((c == 1).all())
        for k in (0, 1):
            for name, v in banks[k].items():
                assert torch.equal(v, before[k][name]), (bad, k, name)


# ---------------------------------------------------------------- GraphActor --
def _agent(cuda, stateful=False):
    agent = attention.Agent(A, grid=(11, 11), stateful_core=stateful)
    detinit.load_into(agent, detinit.deterministic_params(0, A, 4))
    return agent.to(cuda)


def test_graph_actor_records_its_own_steps(cuda):
    """B = 2, 84x84, T = 3, five steps on the fp32 chain, seed 9, as rows [0, 2) of a Bu = 4
    collector; a second actor fills rows [2, 4).  The recorded frames, actions and logp are
    each actor's own per-step outputs, exactly; a recorder-less actor with the first one's
    seed and frames gives bit-identical actions, logits and final h (recording perturbs
    nothing); and an actor's steps leave the other's rows alone."""
    from aaa_amd.policy import GraphActor
    from aaa_amd.unroll import UnrollCollector
    T, B, n = 3, 2, 5
    agent = _agent(cuda)
    col = UnrollCollector(T, 4, 84, 84, cuda)
    ga = GraphActor(agent, 84, 84, B=B, seed=9, chain=True, recorder=col.rows(0, B))
    ga2 = GraphActor(agent, 84, 84, B=B, seed=4, chain=True, recorder=col.rows(B, B))
    plain = GraphActor(agent, 84, 84, B=B, seed=9, chain=True)
    assert ga.recorder.pos.tolist() == [0, 0, 0, 0] and ga.recorder.steps == 0   # the warm-up does not count
    for bank in col.banks:   # (the warm-up steps wrote here)
        for name, v in bank.items():
            if v is not None:
                v.fill_(SENT_U8 if v.dtype == torch.uint8 else SENT_I32 if v.dtype == torch.int32 else SENT_F32)
    frames = [detinit.frames_u8(50, (n, B, 84, 84, 3)), detinit.frames_u8(51, (n, B, 84, 84, 3))]
    outs = [[], []]
    pouts = []
    units = []
    for s in range(n):
        for i, g in enumerate((ga, ga2)):
            a = g.step(frames[i][s])
            outs[i].append((a.clone(), g.log_prob.clone(), g.logits.clone()))
            if s == 0 and i == 0:   # before the second actor's first step: its rows hold the sentinel
                assert bool((col.banks[0]["frames"][:, B:] == SENT_U8).all())
                assert bool((col.banks[0]["actions"][:, B:] == SENT_I32).all())
                assert bool((col.banks[0]["h0"][B:] == SENT_F32).all()) and bool((col.banks[0]["first"][B:] == SENT_F32).all())
                assert bool((col.banks[0]["actions"][0, :B] != SENT_I32).all())
        pa = plain.step(frames[0][s])
        pouts.append((pa.clone(), plain.logits.clone()))
        assert col.ready() == (s in (2, 4))
        if col.ready():
            units.append(col.take(copy=True))
    assert ga.recorder.pos.tolist() == [1, 0, 2, 0] and ga.recorder.completed() == 2 and len(units) == 2
    for u, unroll in enumerate(units):
        s0 = u * (T - 1)
        for i in (0, 1):
            rows = slice(i * B, (i + 1) * B)
            for t in range(T):
                a, lp, _ = outs[i][s0 + t]
                assert torch.equal(unroll.actions[t, rows], a) and torch.equal(unroll.logp[t, rows], lp), (u, i, t)
                assert np.array_equal(unroll.frames[t, rows].cpu().numpy(), frames[i][s0 + t]), (u, i, t)
        assert unroll.rewards.abs().max() == 0 and unroll.done.abs().max() == 0
        assert unroll.first.tolist() == ([1.0] * 4 if u == 0 else [0.0] * 4)
        if u == 0:
            assert float(unroll.initial_state[0].abs().max()) == 0
        else:
            assert all(float(unroll.initial_state[0][r].abs().max()) > 0 for r in range(4))
    assert not torch.equal(units[1].actions[:, :B], units[1].actions[:, B:]) or \
        not torch.equal(units[1].logp[:, :B], units[1].logp[:, B:])            # the two actors really differ
    for s in range(n):                                                           # recording perturbs nothing
        assert torch.equal(pouts[s][0], outs[0][s][0]) and torch.equal(pouts[s][1], outs[0][s][2]), s
    assert torch.equal(plain.h, ga.h) and torch.equal(plain.c, ga.c)
    # reward / done uploaded beside the frame reach the unroll (clip off), from host arrays and device tensors
    col.restart()
    for g in (ga, ga2):
        g.reset()
    for s in range(T):
        ga.step(frames[0][s], reward=np.array([s + 0.5, -s], np.float32), done=np.array([0, s == 1]))
        ga2.step(frames[1][s], reward=torch.tensor([7.0, 8.0], device=cuda), done=None)
    u = col.take()
    assert u.rewards[:T - 1].tolist() == [[1.5, -1.0, 7.0, 8.0], [2.5, -2.0, 7.0, 8.0]]
    assert u.done[:T - 1].tolist() == [[0, 1.0, 0, 0], [0, 0, 0, 0]] and u.first.tolist() == [1.0] * 4
    with pytest.raises(RuntimeError, match="no finished unroll"):
        col.take()


# ----------------------------------------------------------------- continuity --
@pytest.mark.parametrize("stateful", [False, True])
def test_learner_unroll_continues_the_actor(cuda, stateful):
    """The learner recomputes an unroll from the state the actor recorded before its step 0:
    the second completed unroll (all done = 0, so that state is not zero) through
    Learner.step(initial_state=) gives the actor's own per-step logits at 1e-4 -- the bound
    test_actor_chain_matches_learner_forward holds the chain to against aaa_forward -- and
    log_softmax(logits)[a] is the recorded logp within 2e-4 max|logits| (log-softmax is
    2-Lipschitz in the max norm).  Without initial_state the same call misses the step-0
    logits by at least 20 times that bound (CPU oracle, detinit seed 0, these frames:
    miss 1.5e-3 / bound 6e-6 without the stateful core, 1.5e-2 / 8e-6 with it).  With an
    episode end planted on row 0 at t = T-1 of the first unroll, the second one has
    first[0] = 1 and h0[0] = 0, and train_on runs end to end."""
    from aaa_amd.learner import Learner
    from aaa_amd.policy import GraphActor
    from aaa_amd.unroll import UnrollCollector
    T, B, n = 3, 2, 5
    agent = _agent(cuda, stateful)
    learner = Learner(B=B, T=T, frames_u8=True, device=cuda, seed=0, stateful_core=stateful)
    col = UnrollCollector(T, B, 84, 84, cuda, stateful_core=stateful)
    ga = GraphActor(agent, 84, 84, B=B, seed=9, recorder=col.rows(0, B))
    assert ga.chain and torch.equal(ga.flat, learner.flat)
    frames = detinit.frames_u8(77, (n, B, 84, 84, 3))

    def run(done_at=None):
        logits, units = [], []
        for s in range(n):
            done = np.array([1.0, 0.0], np.float32) if s == done_at else None
            ga.step(frames[s], done=done)
            logits.append(ga.logits.clone())
            if col.ready():
                units.append(col.take(copy=True))
        assert len(units) == 2
        return torch.stack(logits), units

    al, (_, u) = run()
    assert len(u.initial_state) == (4 if stateful else 2)
    assert u.first.tolist() == [0.0, 0.0] and all(float(x.abs().max()) > 0 for x in u.initial_state)
    zeros = torch.zeros(T, B, A, device=cuda)
    lg, _ = learner.step(u.frames, zeros, zeros, initial_state=u.initial_state)
    lg0, _ = learner.step(u.frames, zeros, zeros)
    torch.cuda.synchronize()
    ref = al[T - 1:].cpu().numpy()
    mx = float(np.abs(ref).max())
    lgn = lg.cpu().numpy()
    print(f"continuity stateful={stateful}: max|logits| {mx:.4f}, with initial_state max diff "
          f"{float(np.abs(lgn - ref).max()):.3e} (bound {1e-4 * mx:.3e}), without it step-0 miss "
          f"{float(np.abs(lg0[0].cpu().numpy() - ref[0]).max()):.3e}")
    for t in range(T):
        assert_close(lgn[t], ref[t], 1e-4, f"logits t={t}")
    lp = torch.log_softmax(lg, -1).gather(-1, u.actions.long().unsqueeze(-1)).squeeze(-1)
    lperr = float((lp - u.logp).abs().max())
    print(f"  logp max diff {lperr:.3e} (bound {2e-4 * mx:.3e})")
    assert lperr <= 2e-4 * mx, (lperr, 2e-4 * mx)
    miss = float(np.abs(lg0[0].cpu().numpy() - ref[0]).max())
    assert miss >= 20 * 1e-4 * mx, (miss, mx)
    # an episode end at the unroll boundary: the next unroll starts row 0 from reset()
    col.restart()
    ga.reset()
    _, (u0, u1) = run(done_at=T - 1)
    assert u0.done[T - 2].tolist() == [1.0, 0.0] and u1.first.tolist() == [1.0, 0.0]
    for x in u1.initial_state:
        assert float(x[0].abs().max()) == 0 and float(x[1].abs().max()) > 0
    assert learner.opt_steps == 0
    out = learner.train_on(u1, scale=1.0 / (T * B))
    assert learner.opt_steps == 1 and bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(learner.flat).all())
    learner.check_health()
