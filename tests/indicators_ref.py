"""A plain numpy restatement of the technical indicators' definitions (include/pmenv.h,
DESIGN.md "Technical indicators"): f64 throughout, sequential loops over the rows, vectorised
over the columns only, nothing from the library. Every function takes f64 arrays [T, ...]
and returns its outputs [T - L, ..., n_out] from its own first row t = L on. A windowed sum
ascends over its rows from 0.0; `maximum` / `minimum` are numpy's (NaN if either is NaN)."""
import numpy as np

DEFAULTS = {
    "ema": {"timeperiod": 30},
    "bbands": {"timeperiod": 5, "nbdevup": 2.0, "nbdevdn": 2.0},
    "macd": {"fastperiod": 12, "slowperiod": 26, "signalperiod": 9},
    "atr": {"timeperiod": 14},
    "rsi": {"timeperiod": 14},
    "adx": {"timeperiod": 14},
    "dx": {"timeperiod": 14},
    "stoch": {"fastk_period": 5, "slowk_period": 3, "slowd_period": 3},
    "cci": {"timeperiod": 14},
    "obv": {},
    "adosc": {"fastperiod": 3, "slowperiod": 10},
}
OUTPUTS = {"ema": 1, "bbands": 3, "macd": 3, "atr": 1, "rsi": 1, "adx": 1, "dx": 1, "stoch": 2, "cci": 1, "obv": 1,
           "adosc": 1}


def params_of(name, params):
    p = dict(DEFAULTS[name])
    p.update(params)
    return p


def lookback(name, params):
    p = params_of(name, params)
    if name in ("ema", "bbands", "cci"):
        return p["timeperiod"] - 1
    if name == "macd":
        return max(p["fastperiod"], p["slowperiod"]) - 1 + p["signalperiod"] - 1
    if name in ("atr", "rsi", "dx"):
        return p["timeperiod"]
    if name == "adx":
        return 2 * p["timeperiod"] - 1
    if name == "stoch":
        return p["fastk_period"] - 1 + p["slowk_period"] - 1 + p["slowd_period"] - 1
    if name == "obv":
        return 0
    if name == "adosc":
        return max(p["fastperiod"], p["slowperiod"]) - 1
    raise KeyError(name)


def _sum(rows):
    """ascending sum from 0.0 of rows [k, ...]"""
    s = np.zeros(rows.shape[1:])
    for r in rows:
        s = s + r
    return s


def ema(x, p):
    k = 2.0 / (p + 1)
    e = _sum(x[:p]) / p
    out = [e]
    for t in range(p, len(x)):
        e = (x[t] - e) * k + e
        out.append(e)
    return np.stack(out)[..., None]


def bbands(x, p, up, dn):
    out = []
    for t in range(p - 1, len(x)):
        w = x[t - p + 1:t + 1]
        mean = _sum(w) / p
        var = _sum(w * w) / p - mean * mean
        sd = np.where(var > 0.0, np.sqrt(np.where(var > 0.0, var, 0.0)), 0.0)
        out.append(np.stack([mean + up * sd, mean, mean - dn * sd], axis=-1))
    return np.stack(out)


def macd(x, fast, slow, signal):
    if slow < fast:
        fast, slow = slow, fast
    kf, ks, kg = 2.0 / (fast + 1), 2.0 / (slow + 1), 2.0 / (signal + 1)
    ef = _sum(x[slow - fast:slow]) / fast
    es = _sum(x[:slow]) / slow
    m = [ef - es]
    for t in range(slow, len(x)):
        ef = (x[t] - ef) * kf + ef
        es = (x[t] - es) * ks + es
        m.append(ef - es)
    m = np.stack(m)                                   # from t = slow - 1
    sig = _sum(m[:signal]) / signal
    out = [np.stack([m[signal - 1], sig, m[signal - 1] - sig], axis=-1)]
    for i in range(signal, len(m)):
        sig = (m[i] - sig) * kg + sig
        out.append(np.stack([m[i], sig, m[i] - sig], axis=-1))
    return np.stack(out)


def true_range(h, l, c):
    """rows 1 .. T-1 (index t - 1)"""
    return np.maximum(np.maximum(h[1:] - l[1:], np.abs(h[1:] - c[:-1])), np.abs(l[1:] - c[:-1]))


def directional_movement(h, l):
    """(+DM, -DM) of rows 1 .. T-1"""
    up, dn = h[1:] - h[:-1], l[:-1] - l[1:]
    minus = (dn > 0.0) & (up < dn)
    plus = ~minus & (up > 0.0) & (up > dn)
    return np.where(plus, up, 0.0), np.where(minus, dn, 0.0)


def _wilder_avg(v, p):
    """v[i] is the value of row i + 1; from row p on"""
    a = _sum(v[:p]) / p
    out = [a]
    for i in range(p, len(v)):
        a = (a * (p - 1) + v[i]) / p
        out.append(a)
    return np.stack(out)


def atr(h, l, c, p):
    return _wilder_avg(true_range(h, l, c), p)[..., None]


def rsi(x, p):
    d = x[1:] - x[:-1]
    g = _wilder_avg(np.maximum(d, 0.0), p)
    lo = _wilder_avg(np.maximum(x[:-1] - x[1:], 0.0), p)
    den = g + lo
    with np.errstate(all="ignore"):
        out = np.where(np.abs(den) < 1e-8, 0.0, 100.0 * (g / den))
    return out[..., None]


def _wilder_sum(v, p):
    """v[i] is the value of row i + 1: plain sums over rows 1 .. p-1, then S = S - S/p + v from row p on"""
    s = _sum(v[:p - 1])
    out = []
    for i in range(p - 1, len(v)):
        s = s - s / p + v[i]
        out.append(s)
    return np.stack(out)


def _dx(h, l, c, p):
    plus, minus = directional_movement(h, l)
    sp, sm, st = _wilder_sum(plus, p), _wilder_sum(minus, p), _wilder_sum(true_range(h, l, c), p)
    with np.errstate(all="ignore"):
        dip, dim = 100.0 * (sp / st), 100.0 * (sm / st)
        tot = dim + dip
        val = 100.0 * (np.abs(dim - dip) / tot)
        val = np.where(np.abs(tot) < 1e-8, 0.0, val)
        return np.where(np.abs(st) < 1e-8, 0.0, val)     # from row p on


def dx(h, l, c, p):
    return _dx(h, l, c, p)[..., None]


def adx(h, l, c, p):
    d = _dx(h, l, c, p)
    a = _sum(d[:p]) / p
    out = [a]
    for i in range(p, len(d)):
        a = (a * (p - 1) + d[i]) / p
        out.append(a)
    return np.stack(out)[..., None]


def stoch(h, l, c, fk, sk, sd):
    fast = []
    for t in range(fk - 1, len(c)):
        hh, ll = h[t - fk + 1], l[t - fk + 1]
        for i in range(t - fk + 2, t + 1):
            hh, ll = np.maximum(hh, h[i]), np.minimum(ll, l[i])
        with np.errstate(all="ignore"):
            fast.append(np.where(hh == ll, 0.0, (c[t] - ll) / ((hh - ll) / 100.0)))
    fast = np.stack(fast)
    slowk = np.stack([_sum(fast[i - sk + 1:i + 1]) / sk for i in range(sk - 1, len(fast))])
    slowd = np.stack([_sum(slowk[i - sd + 1:i + 1]) / sd for i in range(sd - 1, len(slowk))])
    return np.stack([slowk[sd - 1:], slowd], axis=-1)


def cci(h, l, c, p):
    tp = (h + l + c) / 3.0
    out = []
    for t in range(p - 1, len(tp)):
        w = tp[t - p + 1:t + 1]
        mean = _sum(w) / p
        md = _sum(np.abs(w - mean)) / p
        with np.errstate(all="ignore"):
            out.append(np.where((tp[t] == mean) | (md == 0.0), 0.0, (tp[t] - mean) / (0.015 * md)))
    return np.stack(out)[..., None]


def obv(c, v):
    s = v[0]
    out = [s]
    for t in range(1, len(c)):
        s = s + np.where(c[t] > c[t - 1], v[t], np.where(c[t] < c[t - 1], -v[t], 0.0))
        out.append(s)
    return np.stack(out)[..., None]


def adosc(h, l, c, v, fast, slow):
    kf, ks = 2.0 / (fast + 1), 2.0 / (slow + 1)
    hl = h - l
    with np.errstate(all="ignore"):
        inc = np.where(hl > 0.0, ((c - l) - (h - c)) / hl * v, 0.0)
    ad = inc[0]
    ef = es = ad
    out = [ef - es]
    for t in range(1, len(c)):
        ad = ad + inc[t]
        ef = kf * ad + (1.0 - kf) * ef
        es = ks * ad + (1.0 - ks) * es
        out.append(ef - es)
    return np.stack(out)[max(fast, slow) - 1:][..., None]


def run_op(name, params, o, h, l, c, v):
    """the outputs of one op [T - L_op, ..., n_out] in f64"""
    p = params_of(name, params)
    with np.errstate(invalid="ignore", over="ignore"):
        if name == "ema":
            return ema(c, p["timeperiod"])
        if name == "bbands":
            return bbands(c, p["timeperiod"], float(p["nbdevup"]), float(p["nbdevdn"]))
        if name == "macd":
            return macd(c, p["fastperiod"], p["slowperiod"], p["signalperiod"])
        if name == "atr":
            return atr(h, l, c, p["timeperiod"])
        if name == "rsi":
            return rsi(c, p["timeperiod"])
        if name == "adx":
            return adx(h, l, c, p["timeperiod"])
        if name == "dx":
            return dx(h, l, c, p["timeperiod"])
        if name == "stoch":
            return stoch(h, l, c, p["fastk_period"], p["slowk_period"], p["slowd_period"])
        if name == "cci":
            return cci(h, l, c, p["timeperiod"])
        if name == "obv":
            return obv(c, v)
        if name == "adosc":
            return adosc(h, l, c, v, p["fastperiod"], p["slowperiod"])
    raise KeyError(name)


def indicators(bars, spec, channels=(0, 1, 2, 3, 4)):
    """bars [T, N, C] f32, spec [(name, params)] -> (f64 [T - L, N, K], L): every op aligned to
    the largest lookback L of the call. A channel index of -1 stands for a column no op reads."""
    cols = [np.asarray(bars[..., ch], dtype=np.float64) if ch >= 0 else np.zeros(bars.shape[:-1]) for ch in channels]
    L = max(lookback(n, p) for n, p in spec)
    outs = []
    for name, params in spec:
        res = run_op(name, params, *cols)
        assert res.shape[0] == bars.shape[0] - lookback(name, params) and res.shape[-1] == OUTPUTS[name], name
        outs.append(res[L - lookback(name, params):])
    return np.concatenate(outs, axis=-1), L
