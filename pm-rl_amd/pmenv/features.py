"""The loader's feature stages on the device ("needed for real-data configs").

The reference never feeds its env raw bars. Its loader turns them into observation
channels in four stages:

    reference                                              here
    prices = close[1:] / close[:-1]; rows 1:               build() step 1 — the relatives become a table
      (data/instrument.py:79-80)                             of their own, MarketSeries.relatives
    FixedFracDiff.fit_transform (data/ffd.py:36-57,        ffd_weights (host, ffd_plan.h) + frac_diff
      80-89; instrument.py:257-281; the one piece of         (pmenv_ffd_apply: every column in one launch,
      the reference that runs on the GPU, ffd.py:16-18)      per-column widths, f64 chains)
    split with a purge (instrument.py:284-315,             build() step 3
      instrument_pool.py:380-403)
    MinMaxScaler / StandardScaler per (ticker, feature)    scale (pmenv_scale_fit / pmenv_scale_apply)
      column (instrument.py:318-336, config/base.py:25)

After those stages the close column is a differenced value scaled to 0..1: dividing two
of them is no price relative, so a series built here carries its relatives, and the step
and the compact rollout buffer read that table (trading_env.py, rollout_buffer.py).

Out of scope: the TA-Lib indicators and the ADF search for d (ffd.py:59-78) — the caller
supplies indicator columns as channels and the d values, as the reference loads them from
its d_opt pickles.
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


def build(raw, d, thres=1e-5, train_ratio=0.8, scaler="minmax", close_channel=3, device=None):
    """The reference loader's order on the device. raw [T, N, C] (numpy or torch): C market
    channels per asset, raw prices in `close_channel`; d: a scalar, [C] or [N, C] orders of
    differencing, 0 = leave the channel alone (the reference's feat_ignore columns);
    scaler "minmax", "standard" or None.

      1. relatives[t] = close[t+1] / close[t] and the features are rows 1: (instrument.py:79-80)
      2. FFD of the features; features and relatives lose the first max_width rows, the one
         largest width over all assets and channels (ffd.py:81-88, instrument_pool.py:350-359)
      3. split at int(train_ratio * len) with a purge of max_width rows in front of the test
         part (instrument.py:303-313 with lookback_length = max_width)
      4. each part scaled on its own, per (asset, channel) column (instrument.py:331-336)

    Returns (train, test): MarketSeries whose .relatives [T', N] row t belongs to bars[t],
    with .widths (int32 [N, C]) and .max_width.

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
        s.widths, s.max_width = widths, mw
        parts.append(s)
    return tuple(parts)
