"""The unroll recorder's contract, on its numpy restatement (tests/unroll_ref.py),
driven by a synthetic actor: frame bytes, action, logp, reward and the state
are functions of the environment step and the row, so every slot of every
completed unroll can be named.  T = 3 and 4, 3T + 2 steps, with episode ends
planted at steps that hit t = 1, t = T-2 and t = T-1 of an unroll."""
import numpy as np
import pytest

from unroll_ref import UnrollRef, clip_reward, completed_unrolls, new_bank

B, BU, B0, FB, SF = 3, 5, 1, 20, 8
SENT_U8, SENT_I32, SENT_F32 = 0xA5, -77, -123.5


def _frame(s):
    return ((7 * s + 3 * np.arange(B)[:, None] + np.arange(FB)[None, :]) % 251).astype(np.uint8)


def _action(s):
    return (10 * s + np.arange(B)).astype(np.int32)


def _logp(s):
    return (-(s + np.arange(B) / 8.0)).astype(np.float32)


def _reward(s):
    """What arrives WITH step s (the result of step s-1's action): beyond +-1 from step 4 on."""
    return ((s - 3.5) * (1 + 0.25 * np.arange(B)) * (-1.0) ** s).astype(np.float32)


def _slot_of(s, T):
    return s if s < T else (s - 1) % (T - 1) + 1


def _stream(T, N):
    """done_in per step (the first step starts every episode; ends planted at t = 1, T-2, T-1 on
    different rows) and, from a model of its own, the post-reset state before every step."""
    done = np.zeros((N, B), np.float32)
    done[0] = 1.0
    hits = {}
    for s in range(T, N):   # past the first unroll, so the previous bank is in play too
        hits.setdefault(_slot_of(s, T), s)
    for row, t in enumerate((1, T - 2, T - 1)):
        done[hits[t], row] = 1.0
    pre = np.zeros((N, B, SF), np.float32)
    after = np.full((B, SF), 9.0, np.float32)   # whatever was there before the first episode
    for s in range(N):
        pre[s] = np.where(done[s][:, None] != 0, 0.0, after)
        after = pre[s] + np.float32(s + 1) + 0.5 * np.arange(B, dtype=np.float32)[:, None] + \
            np.arange(SF, dtype=np.float32)[None, :] / 16
    return done, pre, hits


@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("T", [3, 4])
def test_every_completed_unroll_is_the_stream(T, clip):
    N = 3 * T + 2
    done, pre, hits = _stream(T, N)
    assert {1, T - 2, T - 1} <= set(hits)
    banks = [new_bank(T, BU, FB, SF, 0, SENT_U8, SENT_I32, SENT_F32) for _ in (0, 1)]
    ref = UnrollRef(T, B, BU, B0, FB, SF, 0, clip, banks)
    rows = slice(B0, B0 + B)
    h = np.full((B, SF), 9.0, np.float32)
    c = -h
    checked = 0
    for s in range(N):
        ref.begin(done[s], h, c)
        assert np.array_equal(h, pre[s]) and np.array_equal(c, -pre[s])
        inc = np.float32(s + 1) + 0.5 * np.arange(B, dtype=np.float32)[:, None] + \
            np.arange(SF, dtype=np.float32)[None, :] / 16
        h += inc          # the actor's step
        c -= inc
        ref.record(_frame(s), _action(s), _logp(s), _reward(s), done[s])
        assert int(ref.pos[2]) == completed_unrolls(s + 1, T)      # the host formula is the device count
        assert int(ref.pos[0]) == _slot_of(s, T) + 1 if _slot_of(s, T) < T - 1 else int(ref.pos[0]) == 1
        if int(ref.pos[2]) == checked:
            continue
        u, s0 = checked, checked * (T - 1)   # unroll u has just completed: steps s0 .. s0 + T-1
        checked += 1
        assert s == s0 + T - 1 and int(ref.pos[1]) == (u + 1) % 2
        bank = ref.banks[u % 2]
        for t in range(T):
            assert np.array_equal(bank["frames"][t, rows], _frame(s0 + t)), (u, t)
            assert np.array_equal(bank["actions"][t, rows], _action(s0 + t)), (u, t)
            assert np.array_equal(bank["logp"][t, rows], _logp(s0 + t)), (u, t)
        for t in range(T - 1):
            assert np.array_equal(bank["rewards"][t, rows], clip_reward(_reward(s0 + t + 1), clip)), (u, t)
            assert np.array_equal(bank["done"][t, rows], done[s0 + t + 1]), (u, t)
        assert not bank["rewards"][T - 1, rows].any() and not bank["done"][T - 1, rows].any()
        assert np.array_equal(bank["first"][rows], done[s0])
        assert np.array_equal(bank["h0"][rows], pre[s0]) and np.array_equal(bank["c0"][rows], -pre[s0])
        # the next unroll already holds its step 0 and the state before it
        nxt = ref.banks[(u + 1) % 2]
        assert np.array_equal(nxt["frames"][0, rows], _frame(s)) and np.array_equal(nxt["h0"][rows], pre[s])
        assert np.array_equal(nxt["first"][rows], done[s])
    assert checked == completed_unrolls(N, T) >= 3
    if clip:
        assert np.abs(_reward(N - 1)).max() > clip   # the clip had something to clip
    # rows of other actors were never touched
    for bank in ref.banks:
        for name, sent in (("frames", SENT_U8), ("actions", SENT_I32), ("logp", SENT_F32), ("rewards", SENT_F32),
                           ("done", SENT_F32)):
            assert (bank[name][:, [0, 4]] == sent).all(), name
        for name in ("first", "h0", "c0"):
            assert (bank[name][[0, 4]] == np.float32(SENT_F32)).all(), name


def test_planted_episode_ends_reach_the_right_places():
    """T = 4: the end planted at t = T-1 of unroll 1 is ``first`` of unroll 2 and the last ``done`` of
    unroll 1; the one at t = 1 is done[0]; each resets its row's state before the step."""
    T, N = 4, 14
    done, pre, hits = _stream(T, N)
    s_last, s_one = hits[T - 1], hits[1]
    assert _slot_of(s_last, T) == T - 1 and _slot_of(s_one, T) == 1
    assert not pre[s_last, 2].any() and pre[s_last, 0].any()      # row 2 was reset there, row 0 was not
    ref = UnrollRef(T, B, BU, B0, FB, SF)
    h = np.zeros((B, SF), np.float32)
    c = np.zeros((B, SF), np.float32)
    snaps = {}
    for s in range(N):
        ref.begin(done[s], h, c)
        h += 1.0
        ref.record(_frame(s), _action(s), _logp(s), _reward(s), done[s])
        if completed_unrolls(s + 1, T) != completed_unrolls(s, T):
            u = completed_unrolls(s, T)
            snaps[u] = {k: v.copy() for k, v in ref.banks[u % 2].items()}
    u_last = (s_last - (T - 1)) // (T - 1)        # the unroll whose step T-1 is s_last
    assert snaps[u_last]["done"][T - 2, B0 + 2] == 1.0
    assert snaps[u_last + 1]["first"][B0 + 2] == 1.0 and not snaps[u_last + 1]["h0"][B0 + 2].any()
    assert snaps[u_last + 1]["first"][B0 + 0] == 0.0 and snaps[u_last + 1]["h0"][B0 + 0].any()
    u_one = (s_one - 1) // (T - 1)
    assert snaps[u_one]["done"][0, B0 + 0] == 1.0


def test_nan_state_and_nan_reward():
    """A NaN state row is zero after the reset (a select); a NaN reward stays NaN through the clip."""
    ref = UnrollRef(3, B, BU, B0, FB, SF, 0, 1.0)
    h = np.full((B, SF), np.nan, np.float32)
    c = np.ones((B, SF), np.float32)
    ref.begin(np.array([1, 0, 1], np.float32), h, c)
    assert not h[0].any() and np.isnan(h[1]).all() and not h[2].any() and c[1].all() and not c[0].any()
    r = clip_reward(np.array([np.nan, 3.0, -3.0, 0.5], np.float32), 1.0)
    assert np.isnan(r[0]) and list(r[1:]) == [1.0, -1.0, 0.5]
    assert list(clip_reward(np.array([3.0, -3.0], np.float32), 0.0)) == [3.0, -3.0]


def test_host_formula():
    for T in (2, 3, 4, 20):
        n_done = 0
        for n in range(1, 6 * T):
            # step n-1 completes an unroll exactly when it sits in slot T-1
            n_done += _slot_of(n - 1, T) == T - 1
            assert completed_unrolls(n, T) == n_done, (T, n)
