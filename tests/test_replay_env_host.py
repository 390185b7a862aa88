"""`valid_pairs`, the host statement of the per-env replay's valid (start, env) pairs, against
today's per-column definitions (`valid_starts`, `sequence_starts`) on rings with an episode
id per (row, env). No GPU, no torch."""
import numpy as np
import pytest

from replay_env_inputs import bits_of, done_rows, record, ring_rows

W = 4


def column_pairs(ep, oldest, count, H, need_kind, L=None):
    """(st, env) pairs from the per-column lockstep definitions, in (st, env) order."""
    from pmenv.replay import sequence_starts, valid_starts
    out = []
    for b in range(ep.shape[1]):
        col = ep[:, b]
        st = valid_starts(col, oldest, count, W, H) if need_kind == "one" else \
            sequence_starts(col, oldest, count, W, H, L)
        out += [(int(s), b) for s in st]
    out.sort()
    return np.array(out, dtype=np.int64).reshape(-1, 2)


#        B, wrapped
RINGS = [(1, True), (1, False), (70, True), (70, False)]


@pytest.mark.parametrize("B,wrapped", RINGS, ids=[f"B{b}-{'wrapped' if w else 'short'}" for b, w in RINGS])
def test_valid_pairs_is_the_per_column_definition(B, wrapped):
    from pmenv.replay import valid_pairs
    H, rows = ring_rows(W, wrapped)
    ep, head, count = record(done_rows(rows, B, W, seed=B), H)
    oldest = (head - count) % H
    # the fixture's own preconditions
    assert (count == H and oldest > 0) if wrapped else (count < H and oldest == 0)
    assert count > W + 1
    if B > 3:
        chrono = np.roll(ep, -oldest, axis=0)[:count]
        assert (chrono[0, 0] == chrono[-1, 0])                                   # env 0: one episode
        assert (np.diff(chrono[:, 1]) == 1).all()                               # env 1: a new episode every row
        assert set(np.diff(np.flatnonzero(np.diff(chrono[:, 2])))) == {W + 1}    # env 2: episodes of W + 1 rows
        rest = np.diff(chrono[:, 3:], axis=0)
        assert (rest.sum(0) > 0).all() and len(set(rest.sum(0).tolist())) > 3    # the rest: seeded, unequal lengths
    for L in (None, 1, 2, W, 2 * W + 3):
        need = W + 1 if L is None else W + L
        got = valid_pairs(ep, oldest, count, need, H)
        want = column_pairs(ep, oldest, count, H, "one" if L is None else "seq", L)
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (B, wrapped, L)
        if need <= W + 2:
            assert len(got) > 0                                                  # total > 0
        assert (got[:, 0] < max(count - need, 0)).all()
        # (st ascending, env ascending)
        assert (np.diff(got[:, 0] * B + got[:, 1]) > 0).all()
        bits, rowsum = bits_of(got, max(count - need, 0), B)
        assert rowsum[-1] == len(got) and int(sum(bin(int(x)).count("1") for x in bits.reshape(-1))) == len(got)


def test_valid_pairs_with_too_few_rows_is_empty():
    from pmenv.replay import valid_pairs
    H = 4 * W + 9
    for rows in (0, 1, W, W + 1):                                                # count < W + 1 and count == need
        ep, head, count = record(done_rows(rows, 5, W, seed=1), H)
        assert count == rows
        got = valid_pairs(ep, (head - count) % H, count, W + 1, H)
        assert got.shape == (0, 2) and got.dtype == np.int64
    ep, head, count = record(done_rows(W + 2, 5, W, seed=1), H)                  # the first start: env 0 alone has it
    got = valid_pairs(ep, 0, count, W + 1, H)
    assert got[got[:, 1] < 3].tolist() == [[0, 0], [0, 2]]                       # env 1 ends every row: no pair


def test_valid_pairs_hand_cases():
    from pmenv.replay import valid_pairs
    H, count, oldest = 23, 23, 7
    rows = np.arange(count)                                                      # chronological row numbers
    chrono = np.stack([np.zeros(count, np.int32),                                # all equal
                       rows.astype(np.int32),                                    # ends every row
                       (rows // (W + 1)).astype(np.int32),                       # ends every W + 1 rows
                       np.full(count, 9, np.int32)], axis=1)                     # all equal, another id
    ep = np.roll(chrono, oldest, axis=0)
    span = count - (W + 1)
    got = valid_pairs(ep, oldest, count, W + 1, H)
    by_env = {b: got[got[:, 1] == b, 0].tolist() for b in range(4)}
    assert by_env[0] == list(range(span)) and by_env[3] == list(range(span))     # every start
    assert by_env[1] == []                                                       # no pair
    assert by_env[2] == [k for k in range(0, span, W + 1)]                       # exactly one start per episode
    assert len(by_env[2]) == 4 and len(got) > 0
    # a sequence of 2 needs W + 2 rows: an episode of W + 1 rows holds none
    got2 = valid_pairs(ep, oldest, count, W + 2, H)
    assert got2[got2[:, 1] == 2].size == 0 and (got2[:, 1] != 1).all()
    assert got2[got2[:, 1] == 0, 0].tolist() == list(range(count - W - 2))
    # need above count: nothing
    assert valid_pairs(ep, oldest, count, count + 1, H).shape == (0, 2)
    # a [H] array is one column
    assert np.array_equal(valid_pairs(ep[:, 2], oldest, count, W + 1, H)[:, 0], by_env[2])


def test_add_done_and_per_env_signature_are_declared():
    """The Python surface the issue names exists with the documented defaults."""
    import inspect
    from pmenv import replay
    from pmenv.off_policy import OffPolicy
    sig = inspect.signature(replay.DeviceReplay.__init__)
    assert sig.parameters["per_env"].default is False
    assert inspect.signature(replay.DeviceReplay.add).parameters["done"].default is None
    assert inspect.signature(replay.DeviceReplay.indices).parameters["u"].default is None
    assert inspect.signature(replay.DeviceReplay.sequence_indices).parameters["u"].default is None
    assert inspect.signature(OffPolicy.__init__).parameters["episodes"].default is False
    assert hasattr(OffPolicy, "collect_episodes")
    from pmenv import _abi
    names = {s[0] for s in _abi.SIGNATURES}
    assert {"pmenv_replay_valid_build", "pmenv_replay_valid_select", "pmenv_replay_gather_nstep_env",
            "pmenv_replay_gather_seq_env", "pmenv_prio_fill_env"} <= names
