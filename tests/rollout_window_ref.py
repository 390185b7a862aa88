"""The compact rollout's data model (include/pmenv.h, the comment on pmenv_rollout_gather_env)
in numpy, for any F: market channels f < F-1 come from the series, channel F-1 is the
weight ring. Three statements of it, written apart so that each can check the others:

    window_ref    the per-env form, position by position, as the header words it
    lockstep_ref  the lockstep form from an explicit history array (rows of zeros, e0, the w')
    ring_sim      a ring that is updated step by step, as env/sim/weight_buffer.py's is

Host only: no GPU, no library."""
import numpy as np


def window_ref(bars, first, updates, weights, carry, W, ring, t, b):
    """The window (t, b) of pmenv_rollout_gather_env, [N, W, F]; bars [Ts, N, F-1],
    first / updates [T_rec + 1, B], weights [carry + T_rec, B, N]."""
    Ts, N, Fm = bars.shape
    out = np.empty((N, W, Fm + 1), np.float32)
    d0, u = int(first[t, b]), int(updates[t, b])
    for p in range(W):
        d = d0 + p
        out[:, p, :Fm] = bars[d] if 0 <= d < Ts else np.nan
        c = (p - u - 1) % W if ring == "storage" and u >= W - 1 else p
        r = u + c
        if r < W - 1:
            out[:, p, Fm] = 0.0
        elif r == W - 1:
            out[:, p, Fm] = 0.0
            out[0, p, Fm] = 1.0
        else:
            row = carry + t + c - W
            out[:, p, Fm] = weights[row, b] if 0 <= row < weights.shape[0] else 0.0
    return out


def lockstep_ref(bars, start, weights, W, ring, t, b):
    """The window (t, b) of pmenv_rollout_gather, [N, W, F]: window_ref with first = start[b] + t,
    updates = t, carry = 0, built from env b's whole history instead — W-1 rows of zeros, e0,
    then the w' of updates 1 .. T_rec; the window after t updates is rows t .. t+W-1 of it,
    and a full storage ring (t >= W-1) holds update j at position j % W."""
    Ts, N, Fm = bars.shape
    out = np.empty((N, W, Fm + 1), np.float32)
    day = int(start[b]) + t + np.arange(W)
    inside = (day >= 0) & (day < Ts)
    market = np.full((W, N, Fm), np.nan, np.float32)
    market[inside] = bars[day[inside]]
    out[..., :Fm] = market.transpose(1, 0, 2)
    e0 = np.zeros((1, N), np.float32)
    e0[0, 0] = 1.0
    history = np.concatenate([np.zeros((W - 1, N), np.float32), e0, np.asarray(weights, np.float32)[:, b]])
    chrono = history[t:t + W]                               # oldest first: updates t-W+1 .. t (0 is e0)
    if ring == "storage" and t >= W - 1:
        stored = np.empty_like(chrono)
        for c in range(W):
            stored[(t - W + 1 + c) % W] = chrono[c]
        chrono = stored
    out[..., Fm] = chrono.T
    return out


def ring_sim(u, W, N, wts, ring):
    """One env's weight ring after u updates with the rows wts[0 .. u-1] ([>= u, N]), as the
    window shows it, [N, W]. Row 0 is e0 and the write index starts at 1; an update writes at
    the index and advances it modulo W. "storage": the ring as stored once the index has
    wrapped, else the rows written so far behind zero padding. "chrono": the last W rows of
    the history e0, wts[0], .., wts[u-1], zero-padded in front. W >= 2 (index 1 must exist)."""
    assert W >= 2
    buf = np.zeros((W, N), np.float32)
    buf[0, 0] = 1.0
    idx, full = 1, False
    history = [buf[0].copy()]
    for k in range(u):
        buf[idx] = wts[k]
        history.append(np.asarray(wts[k], np.float32))
        idx = (idx + 1) % W
        full = full or idx == 0
    if ring == "storage":
        rows = buf if full else np.concatenate([np.zeros((W - idx, N), np.float32), buf[:idx]])
    else:
        last = history[-W:]
        rows = np.concatenate([np.zeros((W - len(last), N), np.float32), np.stack(last)])
    return np.ascontiguousarray(rows.T)
