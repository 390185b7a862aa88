"""pmenv.replay.sequence_starts — the starts whose sequences of L elements are full length
— against a brute-force scan, and the C ABI's sequence entry point as declared. No GPU."""
import os
import re

import numpy as np
import pytest

W = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def brute_force(row_ep, oldest, count, H, L):
    """Every row of st .. st+L-1+W in one episode, and st + L - 1 < count - W - 1."""
    chrono = [int(row_ep[(oldest + k) % H]) for k in range(count)]
    return [st for st in range(count)
            if st + L - 1 < count - W - 1 and all(chrono[st + k] == chrono[st] for k in range(L + W))]


@pytest.mark.parametrize("L", [1, 2, W, 2 * W + 3])
def test_sequence_starts_match_a_brute_force_scan(L):
    from pmenv.replay import nstep_counts, sequence_starts, valid_starts
    H = 50
    row_ep, head, count = make_ring(H, [30, 3 * W + 8, 2 * W + 6])           # 64 adds: wrapped, three episodes left
    oldest = (head - count) % H
    assert count == H and oldest > 0 and len(set(row_ep)) == 3
    want = brute_force(row_ep, oldest, count, H, L)
    got = sequence_starts(row_ep, oldest, count, W, H, L)
    assert list(got) == want and want
    one = np.asarray(list(valid_starts(row_ep, oldest, count, W, H)))
    m = nstep_counts(row_ep, oldest, count, W, H, one, L)
    assert list(one[m == L]) == want                                         # full length = the n-step count reaches L
    if L == 1:
        assert want == list(one)


def test_sequence_starts_are_empty_when_no_episode_is_long_enough():
    from pmenv.replay import sequence_starts
    row_ep, head, count = make_ring(30, [12, 12])
    assert len(sequence_starts(row_ep, 0, count, W, 30, 12 - W)) == 1        # W + L rows fill an episode exactly
    got = sequence_starts(row_ep, 0, count, W, 30, 12 - W + 1)
    assert len(got) == 0 and not isinstance(got, range)
    assert len(sequence_starts(row_ep, 0, count, W, 30, 1000)) == 0          # longer than the ring
    with pytest.raises(ValueError):
        sequence_starts(row_ep, 0, count, W, 30, 0)


def test_sequence_starts_are_a_range_for_a_single_episode():
    from pmenv.replay import sequence_starts
    row_ep, head, count = make_ring(40, [23])
    for L in (1, 3, 23 - W - 1):
        got = sequence_starts(row_ep, 0, count, W, 40, L)
        assert isinstance(got, range) and got == range(count - W - L)
        assert list(got) == brute_force(row_ep, 0, count, 40, L)
    assert sequence_starts(row_ep, 0, count, W, 40, 23 - W) == range(0)
    row_ep, head, count = make_ring(25, [20, 30])                            # wrapped, one episode left
    oldest = (head - count) % 25
    got = sequence_starts(row_ep, oldest, count, W, 25, 5)
    assert isinstance(got, range) and list(got) == brute_force(row_ep, oldest, count, 25, 5)


def test_abi_declares_the_sequence_entry_point():
    from pmenv import _abi
    assert _abi.PMENV_ABI_VERSION == 4
    header = open(os.path.join(ROOT, "include", "pmenv.h")).read()
    assert re.search(r"#define\s+PMENV_ABI_VERSION\s+4\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+pmenv_replay_gather_seq\s*\(", code)
    sigs = dict((s[0], s) for s in _abi.SIGNATURES)
    seq, nstep = sigs["pmenv_replay_gather_seq"], sigs["pmenv_replay_gather_nstep"]
    assert len(seq[2]) == len(nstep[2]) - 2        # L, time_major for n, gamma; x, a, r, length for six outputs
    lib = _abi.load()
    assert hasattr(lib, "pmenv_replay_gather_seq") and lib.pmenv_abi_version() == 4


def test_load_names_a_symbol_the_library_lacks(monkeypatch):
    from pmenv import _abi
    lib = _abi.load()
    monkeypatch.setattr(_abi, "SIGNATURES", _abi.SIGNATURES + [("pmenv_not_built_yet", None, [])])
    monkeypatch.setattr(_abi, "_lib", None)
    with pytest.raises(ImportError, match="pmenv_not_built_yet") as err:
        _abi.load()
    assert "build.py" in str(err.value)                                      # the rebuild hint
    assert _abi._lib is None                                                 # a failed load caches nothing
    monkeypatch.undo()
    assert _abi._lib is lib and _abi.load() is lib
