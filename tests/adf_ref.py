"""numpy f64 restatement of the ADF definitions of include/pmenv.h, the reference of
test_adf_host.py (which checks it against closed forms and invariances) and test_gpu_adf.py
(which checks the kernels against it) — by np.linalg.lstsq on the uncentred design [1, level,
lagged differences], on purpose another formulation than the kernel's centred normal
equations — the search of ffd.py:59-78 as a plain Python loop over ffd_ref.ffd_ref, and the
catalogue of input series both tests share."""
import functools
import math

import numpy as np

import ffd_ref

OK, TOO_SHORT, DEGENERATE = 0, 1, 2
MIN_ROWS = 16
P_HIGH, P_LOW, D_TOL = 0.05, 0.049, 1e-5


# ---------------------------------------------------------------- the definitions
def maxlag_rule(n):
    """min(n // 2 - 2, ceil(12 (n / 100)^(1/4))), the ceiling in integers"""
    if n < 4:
        return 0
    m = 0
    while 100 * m ** 4 < 20736 * n:
        m += 1
    return min(n // 2 - 2, m)


def maxlag_of(n, maxlag=None):
    return maxlag_rule(n) if maxlag is None else max(0, min(int(maxlag), n // 2 - 2))


def pvalue(s):
    if math.isnan(s):
        return s
    if s > 2.74:
        return 1.0
    if s < -18.83:
        return 0.0
    if s <= -1.61:
        z = 2.1659 + 1.4412 * s + 0.038269 * s * s
    else:
        z = 1.7339 + 0.93202 * s - 0.12745 * s * s - 0.010368 * s ** 3
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def design(x, k, s):
    """(X [nobs, k + 2] = [1, x[i], D[i-1] .. D[i-k]], D[i]) on rows i = s .. n-2"""
    n = len(x)
    D = np.diff(x)
    rows = np.arange(s, n - 1)
    cols = [np.ones(len(rows)), x[rows]] + [D[rows - j] for j in range(1, k + 1)]
    return np.stack(cols, axis=1), D[rows]


def _fit(X, y):
    """(beta, ssr, rank deficient) by lstsq with two steps of iterative refinement on residuals
    taken in np.longdouble: on a unit-root column the level's coefficient is a hundredth of
    the others, and plain lstsq's absolute error — harmless for the fit — is then 1e-13 of the
    statistic, more than the kernel's bound. The refined solution is good to the last bits."""
    beta, _, rank, _ = np.linalg.lstsq(X, y, rcond=None)
    if rank < X.shape[1]:
        return beta, 0.0, True
    Xl, yl, bl = X.astype(np.longdouble), y.astype(np.longdouble), beta.astype(np.longdouble)
    for _ in range(2):
        bl = bl + np.linalg.lstsq(X, (yl - Xl @ bl).astype(np.float64), rcond=None)[0]
    res = yl - Xl @ bl
    return bl.astype(np.float64), float(res @ res), False


def stat_longdouble(x, u):
    """the statistic of the final fit at lag u by another road, all in np.longdouble: the centred
    normal equations solved by Gauss-Jordan elimination. test_adf_host.py holds adf() to it."""
    x = np.asarray(x, dtype=np.float32).astype(np.longdouble)
    n, D = len(x), np.diff(np.asarray(x, dtype=np.float32).astype(np.longdouble))
    rows = np.arange(u, n - 1)
    Xc = np.stack([x[rows]] + [D[rows - j] for j in range(1, u + 1)], axis=1)
    Xc = Xc - Xc.mean(axis=0)
    yc = D[rows] - D[rows].mean()
    p = Xc.shape[1]
    A = np.concatenate([Xc.T @ Xc, (Xc.T @ yc)[:, None], np.eye(p, dtype=np.longdouble)], axis=1)
    for i in range(p):
        A[i] = A[i] / A[i, i]
        for j in range(p):
            if j != i:
                A[j] = A[j] - A[j, i] * A[i]
    res = yc - Xc @ A[:, p]
    return float(A[0, p] / np.sqrt(res @ res / (len(rows) - u - 2) * A[0, p + 1]))


def _bad():
    return dict(stat=math.nan, pvalue=math.nan, usedlag=0, nobs=0, aic_gap=math.inf, kappa=math.nan, tol=math.nan)


def adf(x, maxlag=None, autolag=True):
    """One column: dict of stat, pvalue, usedlag, nobs, status and, for the tests' conditions,
    aic_gap (second-best minus best AIC), kappa (the condition number of the centred,
    column-normalised design of the final fit) and tol (the kernel's bound, below)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = len(x)
    if n < MIN_ROWS:
        return dict(_bad(), status=TOO_SHORT)
    if not np.all(np.isfinite(x)):
        return dict(_bad(), status=DEGENERATE)
    K = maxlag_of(n, maxlag)
    u, gap = K, math.inf
    if autolag and K > 0:
        nobs = n - 1 - K
        aic = []
        for k in range(K + 1):
            X, y = design(x, k, K)
            _, ssr, deficient = _fit(X, y)
            if deficient or not ssr > 0.0:
                return dict(_bad(), status=DEGENERATE)
            aic.append(nobs * math.log(ssr / nobs) + 2.0 * (k + 2))
        u = int(np.argmin(aic))                        # the first of the smallest
        srt = sorted(aic)
        gap = srt[1] - srt[0]
    X, y = design(x, u, u)
    nobs, p = n - 1 - u, u + 2
    beta, ssr, deficient = _fit(X, y)
    if deficient or not ssr > 0.0:
        return dict(_bad(), status=DEGENERATE)
    # [(X'X)^-1]_bb = 1 / (the level's own residual sum of squares on the other columns)
    others = np.delete(X, 1, axis=1)
    _, rss_level, _ = _fit(others, X[:, 1])
    if not rss_level > 0.0:
        return dict(_bad(), status=DEGENERATE)
    stat = beta[1] / math.sqrt(ssr / (nobs - p) / rss_level)
    Xc = X[:, 1:] - X[:, 1:].mean(axis=0)
    Xc = Xc / np.linalg.norm(Xc, axis=0)
    kappa = float(np.linalg.cond(Xc))
    tol = 4.0 * (nobs + 8 * p) * kappa * 2.0 ** -53 * max(1.0, abs(stat))
    return dict(stat=float(stat), pvalue=pvalue(float(stat)), usedlag=u, nobs=nobs, status=OK, aic_gap=gap,
                kappa=kappa, tol=tol)


def adf_columns(y, first=None, maxlag=None, autolag=True):
    """adf of every column of y [R, C] from row first[c] on: dict of arrays"""
    R, C = y.shape
    first = np.zeros(C, dtype=np.int64) if first is None else np.clip(np.asarray(first, dtype=np.int64), 0, R)
    rows = [adf(y[first[c]:, c], maxlag, autolag) for c in range(C)]
    out = {k: np.array([r[k] for r in rows], dtype=np.float64) for k in ("stat", "pvalue", "aic_gap", "kappa", "tol")}
    out.update({k: np.array([r[k] for r in rows], dtype=np.int32) for k in ("usedlag", "nobs", "status")})
    return out


# ---------------------------------------------------------------- the search
def probe(x, d, thres, weights, test=adf):
    """(result of `test` on the column's own T - w + 1 FFD outputs at order d, width)"""
    taps, w = weights(d, thres, len(x))
    if w == 0:
        return test(x), 0
    table, widths = ffd_ref.table_of([taps])
    out = ffd_ref.ffd_ref(np.asarray(x, dtype=np.float32)[:, None], table, widths, w - 1)[:, 0]
    return test(out), w


def search(x, thres, weights, test=adf, d_init=0.0, active=True):
    """ffd.py:59-78 for one column with the contract's two rules (a NaN p ends the column,
    TOO_SHORT counts as p = 1). weights(d, thres, T) -> (taps, width). Returns (d, info): info
    holds ps (every p evaluated), evals, status, pvalue and stat of the last probe."""
    info = dict(ps=[], evals=0, status=OK, pvalue=math.nan, stat=math.nan)
    if d_init > 0.0:
        return float(d_init), info
    if not active:
        return 0.0, info
    low, high, d_opt = 0.0, 1.0, 0.0
    while True:
        d_mid = (low + high) / 2
        if d_mid < D_TOL:
            d_opt = 0.0
            break
        if abs(d_opt - d_mid) < D_TOL:
            break
        d_opt = d_mid
        r, _ = probe(x, d_mid, thres, weights, test)
        info["evals"] += 1
        info["status"], info["pvalue"], info["stat"] = r["status"], r["pvalue"], r["stat"]
        p = 1.0 if r["status"] == TOO_SHORT else r["pvalue"]
        info["ps"].append(p)
        if p > P_HIGH:
            low = d_mid
        elif p < P_LOW:
            high = d_mid
        else:
            break
    return d_opt, info


# ---------------------------------------------------------------- the catalogue
TS = (300, 400)
CS = (1, 5, 64, 65, 130)
KINDS = ("walk", "drift", "ar1_50", "ar1_95", "ar2", "ffd")
FFD_THRES = (1e-2, 3e-3, 1e-3)          # the taps' thresholds of the "ffd" columns: three widths, three firsts
SEED = 20240


def numpy_weights(d, thres, T):
    """pmenv_ffd_weights's rule in numpy (f32 factors, f64 running product, one rounding per tap)"""
    if d == 0.0:
        return np.zeros(0, dtype=np.float32), 0
    k = np.arange(1, T, dtype=np.float32)
    fac = (np.float32(0.0) - np.float32(d + 1.0)) / k + np.float32(1.0)
    w = np.concatenate([[1.0], np.cumprod(fac.astype(np.float64))]).astype(np.float32)
    width = int(np.nonzero(np.abs(w) > np.float32(thres))[0].max())
    return w[:width].copy(), width


def _series(kind, T, rng):
    e = rng.standard_normal(T + 50)
    if kind == "walk":
        x = np.cumsum(e)
    elif kind == "drift":
        x = np.cumsum(e + 0.1)
    elif kind in ("ar1_50", "ar1_95", "ar2"):
        a, b = {"ar1_50": (0.5, 0.0), "ar1_95": (0.95, 0.0), "ar2": (1.2, -0.5)}[kind]
        x = np.zeros(T + 50)
        for t in range(2, T + 50):
            x[t] = a * x[t - 1] + b * x[t - 2] + e[t]
    else:
        raise ValueError(kind)
    return x[50:].astype(np.float32)


@functools.lru_cache(maxsize=None)
def catalogue(T):
    """(y float32 [T, 130], first int32 [130], kinds): column c is of kind KINDS[c % 6]; the rows
    before first[c] hold NaN (they are not part of the column). The smaller cases are the
    leading columns. "ffd" columns are the FFD outputs of a walk at d = 0.3, valid from their
    width - 1 on; the others start at row 0, 3 or 7."""
    rng = np.random.default_rng(SEED + T)
    C = max(CS)
    y = np.empty((T, C), dtype=np.float32)
    first = np.zeros(C, dtype=np.int32)
    kinds = []
    for c in range(C):
        kind = KINDS[c % len(KINDS)]
        kinds.append(kind)
        if kind == "ffd":
            x = _series("walk", T, rng)
            taps, w = numpy_weights(0.3, FFD_THRES[(c // len(KINDS)) % 3], T)
            table, widths = ffd_ref.table_of([taps])
            y[w - 1:, c] = ffd_ref.ffd_ref(x[:, None], table, widths, w - 1)[:, 0]
            first[c] = w - 1
        else:
            y[:, c] = _series(kind, T, rng)
            first[c] = (0, 3, 7)[(c // len(KINDS)) % 3]
        y[:first[c], c] = np.nan
    return y, first, tuple(kinds)


@functools.lru_cache(maxsize=None)
def catalogue_ref(T):
    """adf_columns of the whole catalogue of T rows, computed once"""
    y, first, _ = catalogue(T)
    return adf_columns(y, first)


def search_input(T=400, C=12, seed=7):
    """[T, C] float32 for the find_d tests: walks, drifting walks and AR(1) columns"""
    rng = np.random.default_rng(seed)
    cols = [_series(("walk", "drift", "ar1_95", "ar1_50")[c % 4], T, rng) for c in range(C)]
    return np.stack(cols, axis=1)


# the taps' thresholds of the find_d tests: 1e-2 leaves a 400-row series rows to test at every
# d; at 1e-5 the filters of d <= 0.5 are as wide as the series and their probes TOO_SHORT
SEARCH_THRESES = (1e-2, 1e-5)


@functools.lru_cache(maxsize=None)
def search_ref(thres):
    """the reference search of search_input's columns: (d [C], [info])"""
    x = search_input()
    res = [search(x[:, c], thres, numpy_weights) for c in range(x.shape[1])]
    return np.array([r[0] for r in res]), [r[1] for r in res]
