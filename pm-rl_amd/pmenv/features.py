"""The loader's feature stages on the device ("needed for real-data configs").

The reference never feeds its env raw bars. Its loader turns them into observation
channels in five stages:

    reference                                              here
    InstrumentPool.add_indicators (data_loader.py:37,      indicators (pmenv_ind_apply: the eleven of
      instrument.py:207-232: TA-Lib on the host, once        config/base.py:30-44 over every column in f64,
      per ticker, clipped by the largest lookback)           written into the combined channel tensor)
    prices = close[1:] / close[:-1]; rows 1:               build() step 1 — the relatives become a table
      (data/instrument.py:79-80)                             of their own, MarketSeries.relatives
    FixedFracDiff.fit_transform (data/ffd.py:36-57,        ffd_weights (host, ffd_plan.h) + frac_diff
      80-89; instrument.py:257-281; the one piece of         (pmenv_ffd_apply: every column in one launch,
      the reference that runs on the GPU, ffd.py:16-18)      per-column widths, f64 chains)
    FixedFracDiff.fit (ffd.py:59-78: the bisection of d,   find_d (pmenv_ffd_table, pmenv_adf,
      adfuller per probe, on the host)                       pmenv_adf_search_update: all columns per round)
    split with a purge (instrument.py:284-315,             build() step 3
      instrument_pool.py:380-403)
    MinMaxScaler / StandardScaler per (ticker, feature)    scale (pmenv_scale_fit / pmenv_scale_apply)
      column (instrument.py:318-336, config/base.py:25)

After those stages the close column is a differenced value scaled to 0..1: dividing two
of them is no price relative, so a series built here carries its relatives, and the step
and the compact rollout buffer read that table (trading_env.py, rollout_buffer.py).

The indicators follow the definitions of include/pmenv.h (TA-Lib's default algorithms
restated; DESIGN.md "Technical indicators" lists them and the two deliberate deviations), so
a real-data user needs neither TA-Lib nor a host round trip, and a device-resident series
gets its indicator channels where it lies.

The orders of differencing are searched here too (find_d; build(d="auto")): the reference's
FixedFracDiff.fit (ffd.py:59-78) bisects d per column on the host, one conv1d and one
statsmodels adfuller call per probe, and keeps the result in its d_opt pickles because that is
the slow part of its loader. Here a round is four launches for all columns — the tap table of
every column's d (pmenv_ffd_table), the FFD, a batched augmented Dickey-Fuller test
(pmenv_adf) and the bracket update (pmenv_adf_search_update) — and nothing is read back before
the last round. statsmodels is not a dependency and parity with it is not pinned: the ADF
statistic and the p-value follow the definitions of include/pmenv.h (DESIGN.md "The ADF
search"), with one deliberate deviation: a probe series too short to test (under 16 rows)
counts as p = 1, where the reference would raise.
"""
import ctypes

import numpy as np
import torch

from . import _abi
from .data import MarketSeries


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def ffd_weights(d, thres, T):
    """(taps, width) of order d over a series of T rows (ffd.py:38-47): taps float32
    [width], the filter out[t] = sum_j taps[j] * x[t - j]. d = 0: width 0, the column is
    left alone; d = 1: the single tap [1]. Host only."""
    lib = _abi.load()
    width = ctypes.c_int32(0)
    _abi.check(lib.pmenv_ffd_weights(float(d), float(thres), int(T), None, 0, ctypes.byref(width)), None,
               "pmenv_ffd_weights")
    taps = np.zeros(width.value, dtype=np.float32)
    if width.value:
        _abi.check(lib.pmenv_ffd_weights(float(d), float(thres), int(T), taps.ctypes.data_as(ctypes.c_void_p),
                                         width.value, ctypes.byref(width)), None, "pmenv_ffd_weights")
    return taps, width.value


def ffd_path(T, C, max_width):
    """The kernel pmenv_ffd_apply launches for x [T, C] and its geometry: (name, dict) —
    e.g. ("ffd_apply_kernel<8,8>", {"cw": 64, "slots": 1, "rows": 32, "grid": (345, 4),
    "block": 256, "rb": 8, "jb": 8}); ("", {}) for a refused shape. Host only."""
    text = _abi.load().pmenv_ffd_path(int(T), int(C), int(max_width)).decode()
    if not text:
        return "", {}
    name, *fields = text.split(" ")
    geo = dict(f.split("=") for f in fields)
    out = {k: int(v) for k, v in geo.items() if k != "grid"}
    out["grid"] = tuple(int(v) for v in geo["grid"].split("x"))
    out["rb"], out["jb"] = (int(v) for v in name[name.index("<") + 1:-1].split(","))
    return name, out


def tap_table(d, thres, T, shape):
    """Host side of frac_diff: d (scalar or broadcastable to the column shape) -> (table
    float32 [max_width, C], widths int32 [C], max_width). One weight computation per distinct d."""
    ds = np.broadcast_to(np.asarray(d, dtype=np.float64), shape).reshape(-1)
    cache = {}
    for v in np.unique(ds):
        cache[float(v)] = ffd_weights(float(v), thres, T)
    widths = np.array([cache[float(v)][1] for v in ds], dtype=np.int32)
    mw = int(widths.max()) if widths.size else 0
    table = np.zeros((mw, ds.size), dtype=np.float32)
    for c, v in enumerate(ds):
        taps, w = cache[float(v)]
        table[:w, c] = taps
    return table, widths, mw


def ffd_apply(x, table, widths, max_width, out=None):
    """pmenv_ffd_apply on device tensors: x [T, C] f32, table [max_width, C] f32, widths [C]
    int32 -> out [T - max_width, C]."""
    lib = _abi.load()
    T, C = x.shape
    if out is None:
        out = torch.empty(max(T - max_width, 0), C, dtype=torch.float32, device=x.device)
    _abi.check(lib.pmenv_ffd_apply(_ptr(x), T, C, _ptr(table) if max_width else None, _ptr(widths), int(max_width),
                                   _ptr(out), _stream(x.device)), None, "pmenv_ffd_apply")
    return out


def frac_diff(x, d, thres=1e-5):
    """Fixed-width-window fractional differencing of every column of x [T, ...] (device,
    f32) by its own order: d is a scalar or broadcastable to x.shape[1:], 0 = leave the
    column alone. Returns (out [T - max_width, ...], widths int32 x.shape[1:], max_width):
    every column is clipped by the one largest width of the call (ffd.py:81-88)."""
    x = torch.as_tensor(x)
    if not x.is_cuda:
        x = x.to("cuda")
    x = x.to(torch.float32).contiguous()
    T, cols = x.shape[0], tuple(x.shape[1:])
    table, widths, mw = tap_table(d, thres, T, cols)
    if mw >= T:
        raise ValueError(f"the widest filter ({mw} taps) leaves no row of a {T}-row series")
    tab = torch.from_numpy(table).to(x.device)
    wd = torch.from_numpy(widths).to(x.device)
    out = ffd_apply(x.reshape(T, -1), tab, wd, mw)
    return out.reshape((T - mw,) + cols), wd.reshape(cols), mw


def ffd_table(d, thres, T, cap, taps=None, widths=None):
    """pmenv_ffd_table: d float64 [C] on the device -> (taps float32 [cap, C] with the rows from
    a column's width on zeroed, widths int32 [C]): pmenv_ffd_weights(d[c], thres, T) per column,
    bit for bit, without a host round trip."""
    lib = _abi.load()
    if not torch.is_tensor(d) or not d.is_cuda or d.dtype != torch.float64 or not d.is_contiguous() or d.dim() != 1:
        raise ValueError("d must be a contiguous float64 [C] device tensor")
    C = d.shape[0]
    if taps is None:
        taps = torch.empty(cap, C, dtype=torch.float32, device=d.device)
    if widths is None:
        widths = torch.empty(C, dtype=torch.int32, device=d.device)
    _abi.check(lib.pmenv_ffd_table(_ptr(d), float(thres), int(T), C, int(cap), _ptr(taps) if cap else None,
                                   _ptr(widths), _stream(d.device)), None, "pmenv_ffd_table")
    return taps, widths


def adf_path(R, C, maxlag=None):
    """The kernels pmenv_adf launches for y [R, C] and their geometry, in launch order:
    [("adf_sums_kernel", {"tile": 8, "chunk": 256, "kcap": 17, "grid": 17, "block": 512}),
    ("adf_solve_kernel", {"kcap": 17, "lds": 3952, "grid": 130, "block": 64})]; [] for a refused
    shape. Host only."""
    text = _abi.load().pmenv_adf_path(int(R), int(C), -1 if maxlag is None else int(maxlag)).decode()
    out = []
    for part in text.split(" | ") if text else ():
        name, *fields = part.split(" ")
        out.append((name, {k: int(v) for k, v in (f.split("=") for f in fields)}))
    return out


def adf(y, first=None, maxlag=None, autolag=True, out=None, work=None):
    """The augmented Dickey-Fuller test of every column of y [R, ...] (device, f32; a 2-D y may
    be a view with a row stride), adfuller(x)'s defaults as include/pmenv.h defines them:
    constant only, AIC lag choice up to maxlag (None: the default rule per column), MacKinnon's
    p-value. first (int32, y.shape[1:]): column c is rows first[c] .. R-1. Returns a dict of
    stat, pvalue (float64), usedlag, nobs, status (int32; _abi.ADF_STATUS), each y.shape[1:]."""
    lib = _abi.load()
    if not torch.is_tensor(y) or not y.is_cuda or y.dtype != torch.float32 or y.dim() < 1:
        raise ValueError("y must be a float32 device tensor [R, ...]")
    if y.dim() == 2 and y.stride(1) == 1 and y.stride(0) >= y.shape[1]:
        ld = y.stride(0)
    else:
        y = y.contiguous()
        ld = int(np.prod(y.shape[1:], dtype=np.int64)) if y.dim() > 1 else 1
    R, cols = y.shape[0], tuple(y.shape[1:])
    C = int(np.prod(cols, dtype=np.int64)) if cols else 1
    dev = y.device
    if first is not None:
        first = torch.as_tensor(first, device=dev).to(torch.int32).contiguous()
        if first.numel() != C:
            raise ValueError(f"first must hold one row index per column ({C})")
    ml = -1 if maxlag is None else int(maxlag)
    if ml < -1:
        raise ValueError("maxlag must be None or >= 0")
    nbytes = lib.pmenv_adf_workspace(R, C, ml)
    if work is None:
        work = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    if out is None:
        out = {k: torch.empty(cols, dtype=torch.float64, device=dev) for k in ("stat", "pvalue")}
        out.update({k: torch.empty(cols, dtype=torch.int32, device=dev) for k in ("usedlag", "nobs", "status")})
    _abi.check(lib.pmenv_adf(_ptr(y), R, C, ld, _ptr(first) if first is not None else None, ml, int(bool(autolag)),
                             _ptr(out["stat"]), _ptr(out["pvalue"]), _ptr(out["usedlag"]), _ptr(out["nobs"]),
                             _ptr(out["status"]), _ptr(work), work.numel() * 8, _stream(dev)), None, "pmenv_adf")
    return out


D_TOL = 1e-5          # ffd.py:62,65: the bisection ends within 1e-5 of 0 or of the last probe
D_ROUNDS = 16         # the k-th probe sits 2^-k from the one before: 2^-17 < 1e-5 ends the 17th round


class _Search:
    """The device state of find_d and one round of it (table -> apply -> adf -> update), every
    buffer allocated up front: a round enqueues kernels only, so it can be captured."""

    def __init__(self, x, thres, d_init=None, mask=None):
        self.lib = _abi.load()
        T, C = x.shape
        dev = x.device
        self.T, self.C, self.cap, self.thres, self.dev = T, C, T - 1, float(thres), dev
        self.xpad = torch.zeros(self.cap + T, C, dtype=torch.float32, device=dev)   # row cap + r is series row r
        self.xpad[self.cap:] = x
        act = np.ones(C, dtype=bool) if mask is None else np.broadcast_to(np.asarray(mask, dtype=bool), (C,)).copy()
        d0 = np.zeros(C) if d_init is None else np.broadcast_to(np.asarray(d_init, dtype=np.float64), (C,)).copy()
        if not np.all(np.isfinite(d0)) or np.any(d0 < 0):
            raise ValueError("d_init must be finite and >= 0")
        act &= ~(d0 > 0)
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
        self.low, self.high, self.d_opt = f64(np.zeros(C)), f64(np.ones(C)), f64(np.where(d0 > 0, d0, 0.0))
        self.active = torch.from_numpy(act.astype(np.int32)).to(dev)
        self.evals = torch.zeros(C, dtype=torch.int32, device=dev)
        self.status = torch.zeros(C, dtype=torch.int32, device=dev)
        self.last = torch.full((2, C), float("nan"), dtype=torch.float64, device=dev)
        self.d = torch.empty(C, dtype=torch.float64, device=dev)
        self.taps = torch.empty(self.cap, C, dtype=torch.float32, device=dev)
        self.width = torch.empty(C, dtype=torch.int32, device=dev)
        self.first = torch.empty(C, dtype=torch.int32, device=dev)
        self.y = torch.empty(T, C, dtype=torch.float32, device=dev)
        self.res = {k: torch.empty(C, dtype=torch.float64, device=dev) for k in ("stat", "pvalue")}
        self.res.update({k: torch.empty(C, dtype=torch.int32, device=dev) for k in ("usedlag", "nobs", "status")})
        nbytes = self.lib.pmenv_adf_workspace(T, C, -1)
        if nbytes == 0:
            raise ValueError(f"a series of {T} rows is outside pmenv_adf's range (lag bound above 64)")
        self.work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

    def update(self, probed):
        r = self.res
        _abi.check(self.lib.pmenv_adf_search_update(
            _ptr(r["pvalue"]) if probed else None, _ptr(r["stat"]) if probed else None,
            _ptr(r["status"]) if probed else None, D_TOL, self.C, _ptr(self.low), _ptr(self.high),
            _ptr(self.d_opt), _ptr(self.active), _ptr(self.evals), _ptr(self.status), _ptr(self.last), _ptr(self.d),
            _stream(self.dev)), None, "pmenv_adf_search_update")

    def table(self):
        ffd_table(self.d, self.thres, self.T, self.cap, self.taps, self.width)

    def round(self):
        """One probe of every column at d: its taps, its own T - w + 1 outputs (the series is
        padded in front by cap rows and filtered with max_width = cap, so output row r is series
        row r and column c is valid from row w_c - 1), their ADF p-value, the bracket's update."""
        self.table()
        ffd_apply(self.xpad, self.taps, self.width, self.cap, out=self.y)
        torch.sub(self.width, 1, out=self.first)
        self.first.clamp_(min=0)
        adf(self.y, first=self.first, out=self.res, work=self.work)
        self.update(True)


def find_d(x, thres=1e-5, d_init=None, mask=None):
    """The orders of differencing of every column of x [T, ...] (device, f32): ffd.py:59-78,
    FixedFracDiff.fit's bisection, for all columns at once on the device — per round the tap
    table of every column's d_mid (pmenv_ffd_table), each column's own T - w + 1 FFD outputs
    (pmenv_ffd_apply), their ADF p-values (pmenv_adf) and the bracket update
    (pmenv_adf_search_update), with no host read before the end. thres is the taps' threshold
    (ffd.py:43); the bisection's own tolerance is the reference's 1e-5. d_init (broadcastable to
    x.shape[1:]): columns with a value > 0 keep it and are not searched; mask (bool, likewise):
    columns it leaves out keep d = 0 (the reference's feat_ignore columns). Returns (d float64
    numpy x.shape[1:], info): info holds pvalue and stat of each column's last probe (NaN if it
    had none), width of its d, evals (probes taken) and status (of the last probe), numpy each."""
    x = torch.as_tensor(x)
    if not x.is_cuda:
        x = x.to("cuda")
    x = x.to(torch.float32).contiguous()
    T, cols = x.shape[0], tuple(x.shape[1:])
    if T < 3:
        raise ValueError("x must have at least 3 rows")
    C = int(np.prod(cols, dtype=np.int64)) if cols else 1
    flat = lambda a: None if a is None else np.broadcast_to(np.asarray(a), cols).reshape(-1)  # noqa: E731
    s = _Search(x.reshape(T, C), thres, flat(d_init), flat(mask))
    s.update(False)
    for _ in range(D_ROUNDS):
        s.round()
    s.table()                                   # the widths of the final d
    d = s.d.cpu().numpy().reshape(cols)
    last = s.last.cpu().numpy()
    info = {"pvalue": last[0].reshape(cols), "stat": last[1].reshape(cols),
            "width": s.width.cpu().numpy().reshape(cols), "evals": s.evals.cpu().numpy().reshape(cols),
            "status": s.status.cpu().numpy().reshape(cols)}
    return d, info


def scale(x, method="minmax", stats=None, out=None):
    """Per-column scaling of x [T, ...] (device, f32): method "minmax" (stats = (min, max))
    or "standard" (stats = (mean, std), ddof 0), NaNs skipped in the fit and passed through.
    stats float64 [2, ...] from an earlier call are applied as they are (test rows with train
    statistics); None fits them on x. out may be x. Returns (y, stats)."""
    lib = _abi.load()
    if method not in _abi.SCALE_METHODS:
        raise ValueError(f"scaler must be one of {sorted(_abi.SCALE_METHODS)}")
    m = _abi.SCALE_METHODS[method]
    if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be a contiguous float32 device tensor")
    T, cols = x.shape[0], tuple(x.shape[1:])
    C = int(np.prod(cols, dtype=np.int64)) if cols else 1
    st = _stream(x.device)
    if stats is None:
        stats = torch.empty((2,) + cols, dtype=torch.float64, device=x.device)
        nbytes = lib.pmenv_scale_workspace(T, C)
        work = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=x.device)
        _abi.check(lib.pmenv_scale_fit(_ptr(x), T, C, m, _ptr(stats), _ptr(work), nbytes, st), None, "pmenv_scale_fit")
    elif stats.dtype != torch.float64 or stats.device != x.device or not stats.is_contiguous() or \
            stats.numel() != 2 * C:
        raise ValueError(f"stats must be a contiguous float64 [2, {C}] tensor on {x.device}")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must match x")
    _abi.check(lib.pmenv_scale_apply(_ptr(x), T, C, m, _ptr(stats), _ptr(out), st), None, "pmenv_scale_apply")
    return out, stats


# name -> (period parameters in pmenv_ind_op.p order, float parameters in .f order, TA-Lib's
# defaults, TA-Lib's output names, the moving-average-type parameters: 0 (SMA) only)
_IND = {
    "ema": (("timeperiod",), (), {"timeperiod": 30}, ("real",), ()),
    "bbands": (("timeperiod",), ("nbdevup", "nbdevdn"), {"timeperiod": 5, "nbdevup": 2.0, "nbdevdn": 2.0},
               ("upperband", "middleband", "lowerband"), ("matype",)),
    "macd": (("fastperiod", "slowperiod", "signalperiod"), (), {"fastperiod": 12, "slowperiod": 26, "signalperiod": 9},
             ("macd", "macdsignal", "macdhist"), ()),
    "atr": (("timeperiod",), (), {"timeperiod": 14}, ("real",), ()),
    "rsi": (("timeperiod",), (), {"timeperiod": 14}, ("real",), ()),
    "adx": (("timeperiod",), (), {"timeperiod": 14}, ("real",), ()),
    "dx": (("timeperiod",), (), {"timeperiod": 14}, ("real",), ()),
    "stoch": (("fastk_period", "slowk_period", "slowd_period"), (),
              {"fastk_period": 5, "slowk_period": 3, "slowd_period": 3}, ("slowk", "slowd"),
              ("slowk_matype", "slowd_matype")),
    "cci": (("timeperiod",), (), {"timeperiod": 14}, ("real",), ()),
    "obv": ((), (), {}, ("real",), ()),
    "adosc": (("fastperiod", "slowperiod"), (), {"fastperiod": 3, "slowperiod": 10}, ("real",), ()),
}


def indicator_ops(spec):
    """spec, a list of (name, params) pairs (a list, not the reference's dict, which keeps one
    "ema" only) -> (pmenv_ind_op array, output names). Names are case-insensitive, missing
    parameters take TA-Lib's defaults; an output called "real" takes the indicator's name and
    every name gets "_" + the given parameter values joined by "_" (instrument.py:227-229):
    "ema_30", "upperband_20", "macd_" for empty params. Only SMA smoothing: a matype other
    than 0 is refused."""
    spec = list(spec)
    if not spec:
        raise ValueError("an indicator spec needs at least one (name, params) pair")
    ops = (_abi.PmenvIndOp * len(spec))()
    names = []
    for op, item in zip(ops, spec):
        name, params = item
        key = str(name).lower()
        if key not in _IND:
            raise ValueError(f"unknown indicator {name!r}; one of {sorted(_IND)}")
        periods, floats, defaults, outs, matypes = _IND[key]
        params = dict(params or {})
        for k, v in params.items():
            if k in matypes:
                if v != 0:
                    raise ValueError(f"{key}: {k}={v!r}: only SMA smoothing (0) is supported")
            elif k not in defaults:
                raise ValueError(f"{key}: unknown parameter {k!r}")
        full = dict(defaults, **{k: v for k, v in params.items() if k in defaults})
        op.kind = _abi.IND_KINDS[key]
        for i, k in enumerate(periods):
            if int(full[k]) != full[k]:
                raise ValueError(f"{key}: {k} must be an integer")
            op.p[i] = int(full[k])
        for i, k in enumerate(floats):
            op.f[i] = float(full[k])
        suffix = "_" + "_".join(f"{v}" for v in params.values())
        names += [(key if o == "real" else o) + suffix for o in outs]
    return ops, names


def indicator_layout(spec):
    """(K, lookback, names) of a spec: the output columns and the rows the stage clips. Host only."""
    ops, names = indicator_ops(spec)
    k, look = ctypes.c_int32(0), ctypes.c_int32(0)
    _abi.check(_abi.load().pmenv_ind_layout(ops, len(ops), ctypes.byref(k), ctypes.byref(look)), None,
               "pmenv_ind_layout")
    return k.value, look.value, names


def indicator_path(T, N, spec):
    """The kernels pmenv_ind_apply launches for bars [T, N, .] and their geometry, in launch
    order: [(name, {key: value})], e.g. [("ind_scan_split_kernel", {"walks": 1, "seg": 78,
    "segs": 64, "grid": (8, 64), "block": 64}), ("ind_window_kernel", {...})]; [] for a
    refused shape. Host only."""
    ops, _ = indicator_ops(spec)
    text = _abi.load().pmenv_ind_path(int(T), int(N), ops, len(ops)).decode()
    out = []
    for part in text.split(" | ") if text else ():
        name, *fields = part.split(" ")
        geo = dict(f.split("=") for f in fields)
        out.append((name, {k: tuple(int(x) for x in v.split("x")) if "x" in v else int(v) for k, v in geo.items()}))
    return out


def indicators(bars, spec, channels=(0, 1, 2, 3, 4), out=None, col0=0):
    """The technical indicators of bars [T, N, C] (device, f32, contiguous): spec is a list of
    (name, params) pairs, channels the indices of open, high, low, close and volume (-1 for
    one no requested op reads). Returns (cols [T - L, N, K], names, L): L is the largest
    lookback of the spec and every op is aligned to series row L + r. out, if given, is a
    contiguous [T - L, N, ldo] tensor whose channels col0 .. col0 + K - 1 are written (the
    others are left alone); cols is then that view."""
    lib = _abi.load()
    if not torch.is_tensor(bars) or not bars.is_cuda or bars.dtype != torch.float32 or not bars.is_contiguous() \
            or bars.dim() != 3:
        raise ValueError("bars must be a contiguous float32 [T, N, C] device tensor")
    ops, names = indicator_ops(spec)
    K, L, _ = indicator_layout(spec)
    T, N, C = bars.shape
    if T <= L:
        raise ValueError(f"the longest lookback ({L} rows) leaves no row of a {T}-row series")
    chan = (ctypes.c_int32 * 5)(*[int(c) for c in channels])
    if out is None:
        out = torch.empty(T - L, N, K, dtype=torch.float32, device=bars.device)
        col0 = 0
    elif out.dim() != 3 or tuple(out.shape[:2]) != (T - L, N) or out.dtype != torch.float32 or \
            not out.is_contiguous() or out.device != bars.device:
        raise ValueError(f"out must be a contiguous float32 [{T - L}, {N}, ldo] tensor on {bars.device}")
    nbytes = lib.pmenv_ind_workspace(T, N, ops, len(ops))
    work = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=bars.device)
    _abi.check(lib.pmenv_ind_apply(_ptr(bars), T, N, C, chan, ops, len(ops), _ptr(out), out.shape[2], int(col0),
                                   _ptr(work), nbytes, _stream(bars.device)), None, "pmenv_ind_apply")
    return out[:, :, col0:col0 + K], names, L


_indicators = indicators      # build()'s `indicators` argument shadows the function


def build(raw, d, thres=1e-5, train_ratio=0.8, scaler="minmax", close_channel=3, device=None, indicators=None,
          channels=(0, 1, 2, 3, 4), channel_names=None, auto_channels=None):
    """The reference loader's order on the device. raw [T, N, C] (numpy or torch): C market
    channels per asset, raw prices in `close_channel`; d: a scalar, [C] or [N, C] orders of
    differencing, 0 = leave the channel alone (the reference's feat_ignore columns), or "auto":
    find_d searches them after steps 1 and 1b over the whole series (InstrumentPool.stationary
    runs before the split) for the channels `auto_channels` names — by default the raw channels
    except the volume channel (channels[4]), none of the indicators', as the reference's
    feat_ignore list leaves volume and the oscillators alone; every other channel keeps d = 0;
    scaler "minmax", "standard" or None.

      1. relatives[t] = close[t+1] / close[t] and the features are rows 1: (instrument.py:79-80)
      1b. with `indicators` (a spec as indicators() takes it; `channels` names the OHLCV
         channels): the K indicator columns are appended after the C raw channels, and features
         and relatives lose the first `lookback` rows (instrument.py:207-232); d then
         broadcasts over the C + K channels. None (the default) skips the stage.
      2. FFD of the features; features and relatives lose the first max_width rows, the one
         largest width over all assets and channels (ffd.py:81-88, instrument_pool.py:350-359)
      3. split at int(train_ratio * len) with a purge of max_width rows in front of the test
         part (instrument.py:303-313 with lookback_length = max_width)
      4. each part scaled on its own, per (asset, channel) column (instrument.py:331-336)

    Returns (train, test): MarketSeries whose .relatives [T', N] row t belongs to bars[t],
    with .widths (int32 [N, C]), .max_width and .d (float64 numpy [N, C], the orders used:
    given or found); with `indicators` also .channel_names (the raw
    channels' names, `channel_names` or "c0" .. , then the indicators') and
    .indicator_lookback.

    Two defects of the reference are not reproduced: Instrument.stationary clips the
    features by the FFD width but leaves `prices` at full length, so row t of the relatives
    no longer belongs to row t of the features; and it clips per ticker by that ticker's own
    width, after which the pool's torch.stack over tickers of unequal length cannot succeed."""
    dev = torch.device(device or "cuda")
    r = torch.as_tensor(np.asarray(raw) if not torch.is_tensor(raw) else raw).to(dev, torch.float32)
    if r.dim() != 3 or r.shape[0] < 3:
        raise ValueError("raw must be [T, N, C] with T >= 3")
    T, N, C = r.shape
    if not 0 <= close_channel < C:
        raise ValueError("close_channel outside the channels")
    close = r[:, :, close_channel]
    rel = (close[1:] / close[:-1]).contiguous()                        # 1
    feats = r[1:].contiguous()
    names, look = None, 0
    if indicators is not None:                                         # 1b
        K, look, ind_names = indicator_layout(indicators)
        if T - 1 <= look:
            raise ValueError(f"the longest lookback ({look} rows) leaves no row of a {T - 1}-row series")
        both = torch.empty(T - 1 - look, N, C + K, dtype=torch.float32, device=dev)
        both[:, :, :C] = feats[look:]
        _indicators(feats, indicators, channels, out=both, col0=C)
        raw_names = list(channel_names) if channel_names is not None else [f"c{i}" for i in range(C)]
        if len(raw_names) != C:
            raise ValueError("channel_names must name the C raw channels")
        names = raw_names + ind_names
        feats, rel = both, rel[look:]
    if isinstance(d, str):
        if d != "auto":
            raise ValueError('d must be numbers or "auto"')
        if auto_channels is None:
            auto_channels = [c for c in range(C) if c != channels[4]]
        mask = np.zeros(feats.shape[2], dtype=bool)
        mask[[int(c) for c in auto_channels]] = True
        d, _ = find_d(feats, thres, mask=mask)
    elif auto_channels is not None:
        raise ValueError('auto_channels goes with d="auto"')
    d = np.broadcast_to(np.asarray(d, dtype=np.float64), tuple(feats.shape[1:])).copy()
    x, widths, mw = frac_diff(feats, d, thres)                         # 2
    rel = rel[mw:]
    n = x.shape[0]
    cut = int(train_ratio * n)                                         # 3
    parts = []
    for lo, hi in ((0, cut), (min(cut + mw, n), n)):
        bars = x[lo:hi].contiguous()
        if scaler is not None and bars.shape[0] > 0:                   # 4
            scale(bars, scaler, out=bars)
        s = MarketSeries(bars, device=dev, relatives=rel[lo:hi].contiguous())
        s.widths, s.max_width, s.d = widths, mw, d
        if names is not None:
            s.channel_names, s.indicator_lookback = names, look
        parts.append(s)
    return tuple(parts)
