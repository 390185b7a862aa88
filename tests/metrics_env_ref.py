"""The per-episode trajectory metrics' restatement and inputs (pmenv_metrics_episodes).

`ref` cuts every env's column at its dones and hands each segment, with V0 / e0 prepended as
include/pmenv.h states, to the oracle's lockstep `trajectory_metrics`: nothing is restated
twice. `batch` overlays nine done classes (env b: class b % 9) on rollout_edge_inputs'
ten value / return classes (b % 10): 9 and 10 are coprime, so B >= 90 meets every
combination, and with B >= 9 T the `single` and `pair` classes put an episode boundary on
every row, whatever way a kernel splits the horizon. test_metrics_env_host.py pins these
claims on the CPU; test_gpu_metrics_episodes.py drives the kernel with them."""
import functools
import warnings

import numpy as np

import rollout_edge_inputs as ri
from oracle import trajectory_metrics as or_metrics

INIT_VALUE = 1.03125                # what a restarted env begins from: above some first values, below others
DONE_CLASSES = ["none", "every", "last_only", "first_only", "single", "pair", "period", "random", "bytes"]
KD = len(DONE_CLASSES)
DCLASS = {name: i for i, name in enumerate(DONE_CLASSES)}
FLAT = ("constant", "zero")         # one repeated excess return: zero deviation

SHAPES = [(1, 1, 1), (2, 63, 5), (3, 64, 30), (5, 65, 7), (7, 130, 257), (8, 129, 30), (9, 90, 3), (64, 700, 30),
          (129, 1300, 4)]
# The kernel's turnover part has three forms: N <= 64 (an env per part of a wave), 64 < N <= 256
# (eb = 256 / N envs per workgroup, one thread per asset, partials through the LDS slab) and
# N > 256 (one env per workgroup, threads stride over the assets). SHAPES reaches the first and
# the last; these reach the middle one with eb = 3 and 2, B no multiple of eb, T below and above
# the slab's 8-row block, and eb = 1 at N = 256.
SLAB_SHAPES = [(5, 70, 65), (8, 129, 100), (19, 95, 128), (9, 66, 256)]
ALL_SHAPES = SHAPES + SLAB_SHAPES


def done_column(T, b, rng):
    """Env b's done bytes [T] (class b % 9, q = b // 9)."""
    c, q = DONE_CLASSES[b % KD], b // KD
    t = np.arange(T)
    if c == "none":
        d = np.zeros(T, bool)
    elif c == "every":
        d = np.ones(T, bool)
    elif c == "last_only":
        d = t == T - 1
    elif c == "first_only":
        d = t == 0
    elif c == "single":
        d = t == q % T
    elif c == "pair":
        d = (t == q % T) | (t == (q + 1) % T)
    elif c == "period":
        d = (t + 1) % (2 + q % 5) == 0
    else:
        d = rng.random(T) < 0.2
    d = d.astype(np.uint8)
    if c == "bytes":
        idx = np.flatnonzero(d)
        d[idx] = np.array([2, 128, 255], np.uint8)[(idx + q) % 3]
    return d


def batch(T, B, N, seed):
    """rollout_edge_inputs.metrics_batch(T, B, N, seed) and dones [T, B] uint8."""
    ret, val, w = ri.metrics_batch(T, B, N, seed)
    rng = np.random.default_rng(seed + 1)
    dones = np.stack([done_column(T, b, rng) for b in range(B)], 1)
    return ret, val, w, np.ascontiguousarray(dones)


def segments(dcol):
    """[(first, last)] in steps 1 .. T of one env's done column."""
    T = dcol.shape[0]
    ends = [int(t) + 1 for t in np.flatnonzero(dcol)]
    if not ends or ends[-1] < T:
        ends.append(T)
    firsts = [1] + [e + 1 for e in ends[:-1]]
    return list(zip(firsts, ends))


def ref(returns, values, weights, dones, init_value, rf, periods):
    """Per env a list of (five values, first, last): the oracle's trajectory_metrics on each
    segment, the value path and the weights led by V0 / the entry weights for the first
    segment and by init_value / e0 for every later one."""
    T, B = returns.shape
    N = weights.shape[2]
    e0 = np.zeros(N, np.float32)
    e0[0] = 1.0
    out = []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for b in range(B):
            eps = []
            for k, (first, last) in enumerate(segments(dones[:, b])):
                v0 = values[0, b] if k == 0 else init_value
                w0 = weights[0, b] if k == 0 else e0
                v = np.concatenate([[v0], values[first:last + 1, b]])[:, None]
                w = np.concatenate([w0[None], weights[first:last + 1, b]])[:, None, :]
                m = or_metrics(returns[first - 1:last, b:b + 1], v, w, rf=rf, periods=periods)[0]
                eps.append((m, first, last))
            out.append(eps)
    return out


def dense(refs, K):
    """ref's lists as the kernel's padded arrays: out [B, K, 5] (NaN past the episodes), span
    [B, K, 2] int32 (0 past them), count [B] int32 (exact, also above K)."""
    B = len(refs)
    out = np.full((B, K, 5), np.nan)
    span = np.zeros((B, K, 2), np.int32)
    count = np.array([len(e) for e in refs], np.int32)
    for b, eps in enumerate(refs):
        for k, (m, first, last) in enumerate(eps[:K]):
            out[b, k] = m
            span[b, k] = first, last
    return out, span, count


def sharpe_compared(refs, K):
    """[B, K] bool: the stored episodes whose Sharpe the GPU test compares. An episode of a
    zero-deviation class (FLAT) is compared only where the restatement's Sharpe is exactly
    +-inf or NaN (its two-pass std gave exactly 0, or n = 1): there the inf / NaN pattern is
    the closed form sign(mean) x inf. Where the restatement's mean of n equal numbers rounded
    and left a std of ~1e-19, its Sharpe is a huge finite number that says nothing: those
    episodes are left out of the Sharpe comparison only. Every other class is compared."""
    B = len(refs)
    keep = np.zeros((B, K), bool)
    for b, eps in enumerate(refs):
        flat = ri.METRIC_CLASSES[b % ri.KM] in FLAT
        for k, (m, _, _) in enumerate(eps[:K]):
            keep[b, k] = not flat or not np.isfinite(m[0])
    return keep


@functools.lru_cache(maxsize=None)
def case(T, B, N):
    """The shape's batch (read-only), computed once."""
    arrs = batch(T, B, N, seed=T * 31 + N)
    for a in arrs:
        a.setflags(write=False)
    return arrs


@functools.lru_cache(maxsize=None)
def case_ref(T, B, N, rf, periods):
    return ref(*case(T, B, N), INIT_VALUE, rf, periods)
