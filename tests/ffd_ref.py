"""numpy restatements of the feature kernels' contracts (include/pmenv.h), shared by
test_features_host.py (which checks them against the goldens) and test_gpu_features.py
(which checks the kernels against them), and the error bounds of those comparisons."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ffd")
EPS32 = 2.0 ** -24


def golden(name):
    g = np.load(os.path.join(GOLDEN, f"ffd_{name}.npz"))
    return {k: g[k] for k in g.files}


def golden_taps(g):
    """the reference's taps per column, tap 0 first"""
    out, off = [], 0
    for w in g["widths"]:
        out.append(g["taps"][off:off + w])
        off += w
    return out


def table_of(taps, widths=None):
    """[max_width, C] tap-major table (zeros past a column's width) and int32 widths"""
    widths = np.array([len(t) for t in taps] if widths is None else widths, dtype=np.int32)
    table = np.zeros((int(widths.max()) if len(widths) else 0, len(taps)), dtype=np.float32)
    for c, t in enumerate(taps):
        table[:widths[c], c] = t[:widths[c]]
    return table, widths


def ffd_ref(x, table, widths, max_width):
    """pmenv_ffd_apply's contract: per output one f64 chain over ascending j (the product of
    two f32 is exact in f64, so `acc += w * x` rounds exactly where fma(w, x, acc) does),
    rounded once to f32; width 0 copies x[t]."""
    T, C = x.shape
    out = np.empty((T - max_width, C), dtype=np.float32)
    x64, w64 = x.astype(np.float64), table.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            w = int(widths[c])
            if w == 0:
                out[:, c] = x[max_width:, c]
                continue
            acc = np.zeros(T - max_width, dtype=np.float64)
            for j in range(w):
                acc += w64[j, c] * x64[max_width - j:T - j, c]
            out[:, c] = acc.astype(np.float32)
    return out


def ffd_bound(x, table, widths, max_width, ref):
    """width * 2^-24 * sum_j |w_j x_{t-j}| + ulp32: the worst case of an f32 dot product of
    `width` terms in any order (the reference's conv1d) against the exact sum."""
    T, C = x.shape
    mass = np.zeros((T - max_width, C))
    ax, aw = np.abs(x.astype(np.float64)), np.abs(table.astype(np.float64))
    for c in range(C):
        for j in range(int(widths[c])):
            mass[:, c] += aw[j, c] * ax[max_width - j:T - j, c]
    return widths[None, :] * EPS32 * mass + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def fsum_stats(col, method):
    """(s0, s1) of one column from math.fsum over its numbers: (min, max) or (mean, std ddof 0)"""
    v = [float(a) for a in col if not math.isnan(a)]
    if not v:
        return math.nan, math.nan
    if method == "minmax":
        return min(v), max(v)
    mean = math.fsum(v) / len(v)
    return mean, math.sqrt(math.fsum((a - mean) ** 2 for a in v) / len(v))


def scale_ref(x, method, stats=None):
    """pmenv_scale_fit / _apply's contract in f64 from exactly summed statistics:
    y = f32((x - s0) / den), den = max - min or std, 1 where that is 0. Returns (y, stats [2, C])."""
    T, C = x.shape
    if stats is None:
        stats = np.array([fsum_stats(x[:, c], method) for c in range(C)], dtype=np.float64).T.reshape(2, C)
    den = stats[1] if method == "standard" else stats[1] - stats[0]
    den = np.where(den == 0.0, 1.0, den)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        y = ((x.astype(np.float64) - stats[0][None, :]) / den[None, :]).astype(np.float32)
    return y, stats


def scale_bound(x, y, stats, method):
    """8 * 2^-24 * (|x| + |min or mean|) / (range or std) + 2^-24 * max(1, |y|): sklearn's f32
    roundings of scale_, min_, the product and the sum."""
    den = stats[1] if method == "standard" else stats[1] - stats[0]
    den = np.where(den == 0.0, 1.0, den)
    return 8 * EPS32 * (np.abs(x.astype(np.float64)) + np.abs(stats[0])[None, :]) / den[None, :] + \
        EPS32 * np.maximum(1.0, np.abs(y.astype(np.float64)))
