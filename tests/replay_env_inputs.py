"""Rings with an episode id per (row, env) for the per-env replay's tests
(test_replay_env_host.py on the CPU, test_gpu_replay_env.py on the device): numpy only.

Every ring has heterogeneous columns — env 0 never ends, env 1 ends every row, env 2 ends
every W + 1 rows, the rest take seeded episode lengths in [1, 3W] — and is simulated row by
row the way `DeviceReplay.add(.., done=)` records: row h takes the current ids, then the
envs whose episode ended move on."""
import numpy as np


def done_rows(rows, B, W, seed):
    """done [rows, B] bool: done[t, b] says env b's episode ended with recorded step t."""
    rng = np.random.default_rng(seed)
    done = np.zeros((rows, B), dtype=bool)
    if B > 1:
        done[:, 1] = True
    if B > 2:
        done[W::W + 1, 2] = True                          # steps W, 2W + 1, ..: episodes of W + 1 rows
    for b in range(3, B):
        t = -1
        while True:
            t += int(rng.integers(1, 3 * W + 1))
            if t >= rows:
                break
            done[t, b] = True
    return done


def record(done, H):
    """The ring after recording done's rows: (env_episode [H, B] int32, head, count)."""
    rows, B = done.shape
    ep = np.zeros((H, B), dtype=np.int32)
    cur = np.zeros(B, dtype=np.int32)
    head = count = 0
    for t in range(rows):
        ep[head] = cur
        cur += done[t]
        head = (head + 1) % H
        count = min(count + 1, H)
    return ep, head, count


def ring_rows(W, wrapped):
    """(H, rows recorded): a ring of 4W + 9 rows, recorded H + W + 2 times (count == H, the
    oldest row mid-array) or H - 3 times (count < H, the oldest row is row 0)."""
    H = 4 * W + 9
    return H, (H + W + 2 if wrapped else H - 3)


def bits_of(pairs, span, B):
    """The bit map and the row prefix sums pmenv_replay_valid_build writes, from the
    enumerated pairs: (bits uint64 [span, ceil(B / 64)], rowsum int64 [span + 1])."""
    WB = (B + 63) // 64
    bits = np.zeros((span, WB), dtype=np.uint64)
    for st, b in pairs:
        bits[st, b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    rowsum = np.zeros(span + 1, dtype=np.int64)
    if len(pairs):
        np.cumsum(np.bincount(pairs[:, 0], minlength=span), out=rowsum[1:])
    return bits, rowsum
