"""The numpy reference of the compact rollout's windows (rollout_window_ref.py) against a ring
that is updated step by step, and its lockstep statement against its per-env one. This is
the independent check of what tests/test_gpu_rollout_gather_edges.py compares the kernels
with. W = 1 is left out: a ring whose write index starts at 1 cannot hold one row; the ABI
admits it, and the GPU tests cover it against the data model alone. No GPU."""
import numpy as np
import pytest

from rollout_window_ref import lockstep_ref, ring_sim, window_ref

WS = (2, 3, 4, 7, 50)
NS = (1, 3)
RINGS = ("storage", "chrono")
F = 4                                                       # three market channels and the weights


def _inputs(W, N):
    rng = np.random.default_rng(100 * W + N)
    T = 3 * W + 1                                           # u = 0 .. 3W+1: the ring wraps three times
    B = 2
    bars = rng.random((W + T + 3, N, F - 1)).astype(np.float32)
    weights = (rng.random((T, B, N)) + 0.5).astype(np.float32)     # > 0: no row looks like padding or e0
    start = np.array([2, -1])                               # env 1's first window begins before day 0
    return bars, weights, start, T, B


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("W", WS)
def test_weight_channel_is_the_ring_after_u_updates(W, N, ring):
    bars, weights, start, T, B = _inputs(W, N)
    tcol = np.arange(T + 1)[:, None]
    first = start[None, :] + tcol
    updates = np.repeat(tcol, B, 1)
    for u in range(T + 1):
        for b in range(B):
            sim = ring_sim(u, W, N, weights[:, b], ring)
            assert sim.shape == (N, W)
            got = window_ref(bars, first, updates, weights, 0, W, ring, u, b)
            assert got.shape == (N, W, F) and got.dtype == np.float32
            assert np.array_equal(got[..., F - 1], sim), (u, b)
            assert np.array_equal(lockstep_ref(bars, start, weights, W, ring, u, b)[..., F - 1], sim), (u, b)
    # an env that restarted: u updates since, at row t > u, behind `carry` earlier rows
    carry = W
    shifted = np.concatenate([np.zeros((carry, B, N), np.float32), weights])
    for u in range(0, T + 1, 3):
        for t in range(u, T + 1, 5):
            upd = np.full((T + 1, B), u)
            got = window_ref(bars, first, upd, shifted, carry, W, ring, t, 0)
            sim = ring_sim(u, W, N, weights[t - u:, 0], ring)       # the w' of steps t-u+1 .. t
            assert np.array_equal(got[..., F - 1], sim), (u, t)


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("W", WS)
def test_lockstep_ref_is_window_ref_under_lockstep_bookkeeping(W, N, ring):
    bars, weights, start, T, B = _inputs(W, N)
    tcol = np.arange(T + 1)[:, None]
    first = start[None, :] + tcol
    updates = np.repeat(tcol, B, 1)
    Ts = bars.shape[0]
    for t in range(T + 1):
        for b in range(B):
            want = window_ref(bars, first, updates, weights, 0, W, ring, t, b)
            got = lockstep_ref(bars, start, weights, W, ring, t, b)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (t, b)
            day = start[b] + t + np.arange(W)
            assert np.array_equal(np.isnan(got[..., :F - 1]).all(axis=(0, 2)), (day < 0) | (day >= Ts))
            assert np.array_equal(got[:, (day >= 0) & (day < Ts), :F - 1],
                                  bars[day[(day >= 0) & (day < Ts)]].transpose(1, 0, 2))


def test_the_sweep_reaches_the_wrap_and_the_padding():
    """The cases the sweep is for exist in it: an unfilled ring, the first full one, and two
    wraps in storage order that differ from the chronological order."""
    W, N = 4, 3
    _, weights, _, T, _ = _inputs(W, N)
    w = weights[:, 0]
    reset = np.zeros((N, W), np.float32)
    reset[0, W - 1] = 1.0                                   # e0 behind W-1 rows of padding
    assert np.array_equal(ring_sim(0, W, N, w, "storage"), reset)
    assert np.array_equal(ring_sim(0, W, N, w, "chrono"), reset)
    assert np.array_equal(ring_sim(W - 1, W, N, w, "storage"), ring_sim(W - 1, W, N, w, "chrono"))
    for u in (W, 2 * W - 1, 2 * W, 3 * W):
        s, c = ring_sim(u, W, N, w, "storage"), ring_sim(u, W, N, w, "chrono")
        assert not np.array_equal(s, c) or u % W == W - 1
        assert np.array_equal(np.roll(c, (u + 1) % W, axis=1), s)          # the same rows, rotated
        assert np.array_equal(c[:, -1], w[u - 1])                          # newest last
