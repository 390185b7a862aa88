"""pmenv.replay.nstep_counts — how many transitions an n-step sample folds — against a
literal restatement of agent/td3/td3.py:92-97 over a per-transition `done` flag. No GPU."""
import numpy as np
import pytest

GAMMA = 0.9


def make_ring(H, episodes):
    """row_episode, head, count after adding episodes of the given lengths to a ring of H."""
    row_ep = np.zeros(H, dtype=np.int64)
    head = count = 0
    for e, length in enumerate(episodes, start=1):
        for _ in range(length):
            row_ep[head] = e
            head = (head + 1) % H
            count = min(count + 1, H)
    return row_ep, head, count


def one_step_valid(chrono, count, W, st):
    """The one-step rule, spelled out: st < count - W - 1 and rows st .. st+W in one episode."""
    return 0 <= st < count - W - 1 and all(chrono[st + t] == chrono[st] for t in range(W + 1))


def td3_fold(buffer, gamma):
    """agent/td3/td3.py:92-97 on a full n_step_buffer of (reward, next_state, done)."""
    reward, next_state, done = buffer[-1]
    for r, s_next, d in reversed(buffer[:-1]):
        reward = r + gamma * reward * (1 - d)
        next_state, done = (s_next, d) if d else (next_state, done)
    return reward, next_state, done


W = 4
RINGS = {
    "one_episode": (40, [23]),
    "several_episodes": (60, [17, 9, 21, 6]),
    "wrapped_once": (30, [14, 11, 19]),            # 44 adds
    "wrapped_twice": (25, [20, 13, 16, 18]),       # 67 adds
    "episode_shorter_than_a_window": (30, [12, 3, 12]),
}


@pytest.mark.parametrize("ring", sorted(RINGS))
@pytest.mark.parametrize("n", [1, 2, W, W + 1, 1000])
def test_nstep_counts_match_td3_fold(ring, n):
    from pmenv.replay import nstep_counts, valid_starts
    H, episodes = RINGS[ring]
    row_ep, head, count = make_ring(H, episodes)
    assert n != 1000 or n > count
    oldest = (head - count) % H
    if ring.startswith("wrapped"):
        assert count == H and oldest > 0
    chrono = [int(row_ep[(oldest + k) % H]) for k in range(count)]
    starts = [st for st in range(count) if one_step_valid(chrono, count, W, st)]
    assert list(valid_starts(row_ep, oldest, count, W, H)) == starts and starts
    m = nstep_counts(row_ep, oldest, count, W, H, np.array(starts), n)
    assert m.dtype == np.int32 and m.shape == (len(starts),)
    rewards = np.random.default_rng(len(ring) + n).standard_normal(count + n + W + 2)
    nn = min(n, count)                             # a longer buffer than the ring folds nothing more
    for st, mj in zip(starts, m):
        # the transition at start k ends its episode iff the next start is not a sample;
        # whatever the buffer holds behind a `done` is cut by the (1 - d) factor
        buf = [(rewards[st + k], st + k + 1, not one_step_valid(chrono, count, W, st + k + 1)) for k in range(nn)]
        R, nxt, _ = td3_fold(buf, GAMMA)
        assert nxt == st + mj, (st, n)
        assert 1 <= mj <= n
        want = sum(GAMMA ** k * rewards[st + k] for k in range(mj))
        assert abs(R - want) <= 1e-12 * max(1.0, abs(want))
    if n == 1:
        assert (m == 1).all()
    if ring == "one_episode":
        assert np.array_equal(m, np.minimum(n, count - W - 1 - np.array(starts)))


def test_nstep_counts_rejects_an_invalid_start():
    from pmenv.replay import nstep_counts
    row_ep, head, count = make_ring(30, [12, 12])
    with pytest.raises(ValueError):
        nstep_counts(row_ep, 0, count, W, 30, np.array([10]), 2)      # rows 10 .. 14 span both episodes
    with pytest.raises(ValueError):
        nstep_counts(row_ep, 0, count, W, 30, np.array([count - W - 1]), 2)


def test_abi_declares_the_nstep_entry_point():
    from pmenv import _abi
    assert _abi.PMENV_ABI_VERSION == 4
    sig = dict((s[0], s) for s in _abi.SIGNATURES)["pmenv_replay_gather_nstep"]
    one = dict((s[0], s) for s in _abi.SIGNATURES)["pmenv_replay_gather"]
    assert len(sig[2]) == len(one[2]) + 7          # row_episode, oldest, count, n, gamma, steps, discount
    assert hasattr(_abi.load(), "pmenv_replay_gather_nstep")
