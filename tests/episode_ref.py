"""Numpy references for the per-env episodes (pmenv_restart_days, pmenv.episodes)."""
import numpy as np


def restart_ref(day, end, restart, W):
    """One restart call's bookkeeping: day[b] is the bar the step just appended.
    Returns (done bool [B], new_day int32 [B])."""
    day, end, restart = (np.asarray(x, dtype=np.int64) for x in (day, end, restart))
    nxt = day + 1
    done = nxt >= end
    return done, np.where(done, restart + W, nxt).astype(np.int32)


def window_ref(series, start, W, F):
    """[B, N, W, F] windows of series [T, N, F-1] from each start day, with the seed of the
    weight channel (1 at n = 0, t = W - 1); days outside the series (or a negative start,
    the whole window) are NaN."""
    series = np.asarray(series, dtype=np.float32)
    T, N, Fm = series.shape
    assert Fm == F - 1
    start = np.asarray(start, dtype=np.int64).reshape(-1)
    out = np.zeros((start.size, N, W, F), np.float32)
    for b, s in enumerate(start):
        for t in range(W):
            d = s + t
            out[b, :, t, :Fm] = series[d] if (s >= 0 and d < T) else np.nan
    out[:, 0, W - 1, Fm] = 1.0
    return out
