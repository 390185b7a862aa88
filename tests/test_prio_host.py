"""pmenv.replay.prio_row_events — the leaves one `add` closes and opens in the priority
tree — simulated over rings against `valid_starts`, and the C ABI's priority entry points
as declared. No GPU."""
import os
import re

import numpy as np
import pytest

W = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def simulate(H, episodes):
    """Add episodes of the given lengths to a ring of H; after every add yield (count,
    the open rows kept from the events, the rows valid_starts names)."""
    from pmenv.replay import prio_row_events, valid_starts
    row_ep = np.zeros(H, dtype=np.int64)
    head = count = 0
    open_rows = set()
    for e, length in enumerate(episodes, start=1):
        for _ in range(length):
            close_row, open_row = prio_row_events(row_ep, head, count, e, W, H)
            row_ep[head] = e
            head = (head + 1) % H
            count = min(count + 1, H)
            if close_row is not None:
                assert close_row == (head - 1) % H              # the row just overwritten
                open_rows.discard(close_row)
            if open_row is not None:
                assert open_row not in open_rows and open_row != close_row
                open_rows.add(open_row)
            oldest = (head - count) % H
            want = {(oldest + int(st)) % H for st in valid_starts(row_ep, oldest, count, W, H)}
            yield count, set(open_rows), want


@pytest.mark.parametrize("H,episodes", [
    (50, [30, 3 * W + 8, 2 * W + 6]),        # test_seq_host.py's ring: 64 adds, wrapped, three episodes left
    (40, [23]),                              # a single episode, not full
    (25, [70]),                              # a single episode, wrapped more than twice
    (30, [W + 1, 12, W, 3, W + 2, 20]),      # episodes shorter than W + 2 never open a row
    (W + 2, [3 * W + 7]),                    # the smallest ring
    (W + 2, [W + 2, W + 3, 1, W + 2]),
], ids=["three-episodes-wrapped", "single", "single-wrapped", "short-episodes", "smallest", "smallest-episodes"])
def test_row_events_keep_the_open_rows_equal_to_valid_starts(H, episodes):
    seen = []
    for count, got, want in simulate(H, episodes):
        assert got == want
        seen.append((count, len(got)))
    counts = [c for c, _ in seen]
    assert min(H, sum(episodes)) == counts[-1]
    if sum(episodes) >= H:
        assert {W + 1, W + 2, H} <= set(counts)              # count passed through W + 1, W + 2 and H
    assert dict(seen).get(W + 1, 0) == 0                     # W + 1 rows hold no start yet


def test_first_start_opens_at_w_plus_two_rows():
    steps = list(simulate(40, [23]))
    assert [len(g) for _, g, _ in steps[:W + 3]] == [0] * (W + 1) + [1, 2]
    assert steps[W + 1][1] == {0}


def test_an_episode_shorter_than_a_window_opens_nothing():
    for H, eps in ((30, [W] * 9), (30, [1] * 40)):
        assert all(not got and not want for _, got, want in simulate(H, eps))
    # W + 1 rows of one episode are a window: its one start opens once a later row exists
    sizes = [len(got) for _, got, _ in simulate(30, [W + 1, W + 1, W + 1])]
    assert sizes[:W + 1] == [0] * (W + 1) and sizes[W + 1] == 1 and max(sizes) == 2


def test_no_event_touches_a_row_twice_or_both_ways():
    from pmenv.replay import prio_row_events
    row_ep = np.ones(10, dtype=np.int64)
    assert prio_row_events(row_ep, 0, 0, 1, W, 10) == (None, None)
    assert prio_row_events(row_ep, W + 1, W + 1, 1, W, 10) == (None, 0)
    assert prio_row_events(row_ep, 3, 10, 1, W, 10) == (3, (3 + 1 + 10 - W - 2) % 10)
    row_ep[:3] = 2                                           # the candidate's window straddles two episodes
    assert prio_row_events(row_ep, 3, 10, 2, W, 10)[1] is None


def test_prio_layout_levels():
    from pmenv.replay import prio_layout
    for leaves, sizes in ((1, [1, 1]), (63, [63, 1]), (64, [64, 1]), (65, [65, 2]), (4096, [4096, 64]),
                          (4097, [4097, 65, 2]), (262145, [262145, 4097, 65, 2]), (16384 * 256, [16384 * 256, 65536, 1024, 16])):
        lay = prio_layout(leaves)
        assert [n for _, n, _ in lay["levels"]] == sizes
        assert lay["levels"][0][0] == 64 and lay["levels"][0][2] == np.float32
        off = 64 + 4 * ((leaves + 63) // 64 * 64)
        for o, n, dt in lay["levels"][1:]:
            assert o == off and o % 8 == 0 and dt == np.float64
            off += 8 * ((n + 63) // 64 * 64)
        assert lay["bytes"] == off


ENTRY_POINTS = {   # name -> the argument list include/pmenv.h declares, as _abi's ctypes
    "pmenv_prio_tree_bytes": "int64_t",
    "pmenv_prio_init": "void* int64_t hipStream_t",
    "pmenv_prio_fill": "void* int64_t int64_t int64_t int64_t hipStream_t",
    "pmenv_prio_sample": "void* int64_t int32_t double* int32_t float int32_t* int32_t* int32_t* float* hipStream_t",
    "pmenv_prio_update": "void* int64_t int32_t* float* int32_t float float hipStream_t",
}


def test_abi_declares_the_priority_entry_points():
    import ctypes
    from pmenv import _abi
    assert _abi.PMENV_ABI_VERSION == 4
    header = open(os.path.join(ROOT, "include", "pmenv.h")).read()
    assert re.search(r"#define\s+PMENV_ABI_VERSION\s+4\b", header)
    for cite in ("td3.py:39", ":118", ":144", "Schaul"):
        assert cite in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    sigs = dict((s[0], s) for s in _abi.SIGNATURES)
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float,
             "hipStream_t": ctypes.c_void_p}
    lib = _abi.load()
    for name, want in ENTRY_POINTS.items():
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, name
        declared = []
        for arg in m.group(2).split(","):
            words = arg.replace("const", "").split()
            declared.append(words[0] if len(words) == 1 or "*" not in arg else words[0].rstrip("*") + "*")
        assert " ".join(declared) == want, name
        _, res, args = sigs[name]
        assert res == (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int)
        assert args == [ctypes.c_void_p if d.endswith("*") else ctype[d] for d in declared], name
        assert hasattr(lib, name)
    assert lib.pmenv_abi_version() == 4


def test_tree_bytes_match_the_documented_layout():
    from pmenv import _abi
    from pmenv.replay import prio_layout
    lib = _abi.load()
    for leaves in (1, 63, 64, 65, 4096, 4097, 262145, 16384 * 256, 2 ** 31 - 1):
        assert lib.pmenv_prio_tree_bytes(leaves) == prio_layout(leaves)["bytes"]
    for leaves in (0, -1, 2 ** 31, 2 ** 40):
        assert lib.pmenv_prio_tree_bytes(leaves) == 0
