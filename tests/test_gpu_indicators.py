"""The technical indicators on the GPU (pmenv.features.indicators; csrc/indicators.h) against
the numpy restatement of their definitions (tests/indicators_ref.py), in both forms of the
recurrences, each asserted by name before any value is compared: every output within one
f32 ulp of f32(restatement) (the bounded oscillators within 1e-9 absolute as well) with at
most 1 + 1e-5 * count elements not bit-equal; obv and the windowed ops bit-equal;
independence of the geometry and of what the workspace held; placement inside a wider
tensor between guard rows; NaN confinement; the refusals; a captured graph replayed on
fresh bars; and build(indicators=...). Needs an MI355X."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import indicators_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = 12345.0
SPLIT_MAX_COLS, SEG_ROWS = 16384, 32          # ind_plan.h: split up to these columns, with T - L >= 2 * SEG_ROWS
NS = (1, 3, 63, 64, 65, 130)
BOUNDED = ("rsi", "dx", "adx", "slowk", "slowd")
BIT_EQUAL = ("obv", "upperband", "middleband", "lowerband", "slowk", "slowd", "cci")

# every op twice, periods 2, 5, 14 and 30, a second op of a kind (a second walk), swapped
# macd periods, unequal band multipliers
FULL = [("ema", {"timeperiod": 30}), ("ema", {"timeperiod": 2}), ("bbands", {"timeperiod": 5}),
        ("bbands", {"timeperiod": 30, "nbdevup": 1.5, "nbdevdn": 0.5}),
        ("macd", {"fastperiod": 5, "slowperiod": 14, "signalperiod": 5}),
        ("macd", {"fastperiod": 14, "slowperiod": 5, "signalperiod": 2}),
        ("atr", {"timeperiod": 14}), ("atr", {"timeperiod": 2}), ("rsi", {"timeperiod": 14}), ("rsi", {"timeperiod": 2}),
        ("adx", {"timeperiod": 14}), ("adx", {"timeperiod": 2}), ("dx", {"timeperiod": 14}), ("dx", {"timeperiod": 5}),
        ("stoch", {}), ("stoch", {"fastk_period": 14, "slowk_period": 5, "slowd_period": 2}),
        ("cci", {"timeperiod": 14}), ("cci", {"timeperiod": 2}), ("obv", {}), ("adosc", {}),
        ("adosc", {"fastperiod": 14, "slowperiod": 5})]
DEFAULT = [(n, {}) for n in ("ema", "bbands", "macd", "atr", "rsi", "adx", "dx", "stoch", "cci", "obv", "adosc")]
L_FULL, L_DEFAULT = 29, 33
CHANS = {5: (0, 1, 2, 3, 4), 7: (5, 2, 6, 0, 3)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def ohlcv(T, N, C, seed=0):
    """[T, N, C] f32 with h >= max(o, c), l <= min(o, c), integer volumes below 2^24 and runs
    of one to four repeated bars, some of them flat (h == l): HH == LL, zero gains and zero
    ranges all occur. The other channels hold noise."""
    rng = np.random.default_rng(1000 * T + 10 * N + C + seed)
    chan = CHANS[C]
    c = 50.0 * np.exp(np.cumsum(0.02 * rng.standard_normal((T, N)), axis=0))
    o = c * np.exp(0.005 * rng.standard_normal((T, N)))
    h = np.maximum(o, c) * (1.0 + 0.01 * np.abs(rng.standard_normal((T, N))))
    lo = np.minimum(o, c) * (1.0 - 0.01 * np.abs(rng.standard_normal((T, N))))
    v = rng.integers(1, 2 ** 24, (T, N)).astype(np.float64)
    bars = (rng.standard_normal((T, N, C)) * 7).astype(np.float32)
    for ch, x in zip(chan, (o, h, lo, c, v)):
        bars[..., ch] = x.astype(np.float32)
    hi_, lo_ = bars[..., chan[1]], bars[..., chan[2]]
    np.maximum(hi_, np.maximum(bars[..., chan[0]], bars[..., chan[3]]), out=hi_)      # the rounding kept the order
    np.minimum(lo_, np.minimum(bars[..., chan[0]], bars[..., chan[3]]), out=lo_)
    for n in range(N):
        t = 1
        while True:
            t += int(rng.integers(3, 40))
            run = int(rng.integers(1, 5))
            if t + run >= T:
                break
            if rng.random() < 0.4:                                   # a flat bar first: o = h = l = c
                for ch in chan[:3]:
                    bars[t - 1, n, ch] = bars[t - 1, n, chan[3]]
            bars[t:t + run, n, :] = bars[t - 1, n, :]
            t += run
    bars.setflags(write=False)
    return bars


@functools.lru_cache(maxsize=None)
def want(T, N, C, spec_id, seed=0):
    spec = FULL if spec_id == "full" else DEFAULT
    out, L = ref.indicators(ohlcv(T, N, C, seed), spec, CHANS[C])
    out.setflags(write=False)
    return out, L


def _names(spec):
    from pmenv import features
    return features.indicator_layout(spec)[2]


def _form(T, N, spec):
    from pmenv import features
    return features.indicator_path(T, N, spec)[0][0]


def _expect_form(T, N, L):
    return "ind_scan_split_kernel" if N <= SPLIT_MAX_COLS and T - L >= 2 * SEG_ROWS else "ind_scan_seq_kernel"


def apply_raw(bars, spec, chan, ldo=None, col0=0, off=0, work_fill=None, rc_want=0, T=None, work_short=0,
              work_off=0, out_ptr=None):
    """pmenv_ind_apply through the raw ABI: bars and out `off` floats past their buffers'
    (256-B aligned) starts, out between guard rows, every float of out preset to SENTINEL.
    Returns (status, out [T - L, N, ldo]); the guards must come back untouched."""
    from pmenv import _abi, features
    lib = _abi.load()
    ops, _ = features.indicator_ops(spec)
    K, L, _ = features.indicator_layout(spec)
    Tb, N, C = bars.shape
    T = Tb if T is None else T
    ldo = K if ldo is None else ldo
    R = max(T - L, 1)
    bb = torch.zeros(bars.size + off + 4, device=DEV)
    bv = bb[off:off + bars.size]
    bv.copy_(torch.from_numpy(np.array(bars, dtype=np.float32).ravel()))
    guard = 2 * N * ldo + 3
    ob = torch.full((guard + off + R * N * ldo + guard,), SENTINEL, device=DEV)
    ov = ob[guard + off:guard + off + R * N * ldo]
    nbytes = lib.pmenv_ind_workspace(T, N, ops, len(ops))
    work = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=DEV)
    if work_fill is not None:
        work.fill_(work_fill) if not isinstance(work_fill, str) else work.copy_(
            torch.from_numpy(np.random.default_rng(5).standard_normal(work.numel()) * 1e30).to(DEV))
    rc = lib.pmenv_ind_apply(ctypes.c_void_p(bv.data_ptr()), T, N, C, (ctypes.c_int32 * 5)(*chan), ops, len(ops),
                             ctypes.c_void_p(ov.data_ptr() if out_ptr is None else out_ptr(bv)), ldo, col0,
                             ctypes.c_void_p(work.data_ptr() + work_off), max(nbytes - work_short, 0),
                             ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == rc_want, rc
    full = ob.cpu().numpy()
    lo = guard + off
    assert np.all(full[:lo] == SENTINEL) and np.all(full[lo + R * N * ldo:] == SENTINEL), "guard rows written"
    return rc, full[lo:lo + R * N * ldo].reshape(R, N, ldo)


def check_values(got, want64, names):
    """the issue's value conditions, per output column"""
    assert got.shape == want64.shape
    w32 = want64.astype(np.float32)
    for k, name in enumerate(names):
        g, w, w64 = got[..., k], w32[..., k], want64[..., k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        ok = ~np.isnan(w)
        g, w, w64 = g[ok], w[ok], w64[ok]
        differ = _bits(g) != _bits(w)
        base = name.split("_")[0]
        print(f"{name}: {int(differ.sum())} of {g.size} not bit-equal, max |err| {np.abs(g - w64).max() if g.size else 0:.3e}")
        if base in BIT_EQUAL:
            assert not differ.any(), name
            continue
        near = (g >= np.nextafter(w, np.float32(-np.inf))) & (g <= np.nextafter(w, np.float32(np.inf)))
        if base in BOUNDED:
            near |= np.abs(g.astype(np.float64) - w64) <= 1e-9
        assert near.all(), (name, int((~near).sum()))
        assert differ.sum() <= 1 + 1e-5 * g.size, (name, int(differ.sum()), g.size)


# ---------------------------------------------------------------- values, both forms
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("form,T", [("ind_scan_split_kernel", 400), ("ind_scan_seq_kernel", L_FULL + 2 * SEG_ROWS - 1)])
def test_every_output_matches_the_restatement(form, T, N):
    C = 7 if N in (3, 64) else 5
    assert _form(T, N, FULL) == form == _expect_form(T, N, L_FULL)            # the form by name before any value
    w, L = want(T, N, C, "full")
    assert L == L_FULL
    _, got = apply_raw(ohlcv(T, N, C), FULL, CHANS[C], off=N % 4)
    check_values(got, w, _names(FULL))


def test_sequential_form_above_the_column_threshold():
    """the many-columns form where the plan takes it on its own: more columns than the split
    form's limit, more than one workgroup column group, a tail group"""
    T, N = 100, SPLIT_MAX_COLS + 37
    assert _form(T, N, DEFAULT) == "ind_scan_seq_kernel" == _expect_form(T, N, L_DEFAULT)
    rng = np.random.default_rng(4)
    base = ohlcv(T, 130, 5)
    bars = np.ascontiguousarray(base[:, rng.integers(0, 130, N), :])
    w, L = ref.indicators(bars, DEFAULT)
    _, got = apply_raw(bars, DEFAULT, CHANS[5])
    check_values(got, w, _names(DEFAULT))


@pytest.mark.parametrize("extra", [1, 2, 2 * SEG_ROWS, 2 * SEG_ROWS + 1, 3 * SEG_ROWS + 5])
@pytest.mark.parametrize("spec_id", ["full", "default"])
def test_shortest_series_and_the_first_split_shapes(spec_id, extra):
    """T = L + 1 (one output row), L + 2, and the first lengths the split form takes"""
    spec = FULL if spec_id == "full" else DEFAULT
    L0 = L_FULL if spec_id == "full" else L_DEFAULT
    T, N = L0 + extra, 65
    assert _form(T, N, spec) == _expect_form(T, N, L0)
    w, L = want(T, N, 5, spec_id)
    assert L == L0 and w.shape[0] == extra
    _, got = apply_raw(ohlcv(T, N, 5), spec, CHANS[5])
    check_values(got, w, _names(spec))


# ---------------------------------------------------------------- geometry, repeatability
@pytest.mark.parametrize("T", [400, L_FULL + 40])
def test_a_column_alone_equals_the_column_among_130(T):
    bars = ohlcv(T, 130, 5)
    form = _form(T, 130, FULL)
    assert form == _form(T, 1, FULL) == _expect_form(T, 1, L_FULL)
    _, all_ = apply_raw(bars, FULL, CHANS[5])
    _, one = apply_raw(np.ascontiguousarray(bars[:, 77:78]), FULL, CHANS[5])
    assert np.array_equal(_bits(one[:, 0]), _bits(all_[:, 77]))


@pytest.mark.parametrize("T", [400, L_FULL + 40])
def test_repeats_and_workspace_contents_do_not_change_a_bit(T):
    bars = ohlcv(T, 65, 5)
    _, first = apply_raw(bars, FULL, CHANS[5], work_fill=0.0)
    for fill in (0.0, float("nan"), "garbage"):
        _, again = apply_raw(bars, FULL, CHANS[5], work_fill=fill)
        assert np.array_equal(_bits(again), _bits(first)), fill


# ---------------------------------------------------------------- placement
@pytest.mark.parametrize("T", [400, L_FULL + 40])
def test_outputs_land_in_their_channels_only(T):
    """ldo > K and col0 > 0: the other channels keep their sentinels, as do the guard rows;
    out and bars sit 4 B past a 16-B boundary"""
    N, C = 63, 7
    K = len(_names(FULL))
    _, tight = apply_raw(ohlcv(T, N, C), FULL, CHANS[C])
    _, wide = apply_raw(ohlcv(T, N, C), FULL, CHANS[C], ldo=K + 5, col0=2, off=1)
    assert np.array_equal(_bits(wide[..., 2:2 + K]), _bits(tight))
    assert np.all(wide[..., :2] == SENTINEL) and np.all(wide[..., 2 + K:] == SENTINEL)


# ---------------------------------------------------------------- NaN confinement
@pytest.mark.parametrize("T", [400, L_FULL + 40])
def test_a_nan_close_stays_in_its_asset(T):
    N, bad, row = 65, 40, T // 2
    clean = ohlcv(T, N, 5)
    bars = clean.copy()
    bars[row, bad, 3] = np.nan
    _, base = apply_raw(clean, FULL, CHANS[5])
    _, got = apply_raw(bars, FULL, CHANS[5])
    others = np.arange(N) != bad
    assert np.array_equal(_bits(got[:, others]), _bits(base[:, others]))
    w, _ = ref.indicators(bars[:, bad:bad + 1], FULL)
    assert np.array_equal(np.isnan(got[:, bad]), np.isnan(w[:, 0]))
    assert np.array_equal(np.isinf(got[:, bad]), np.isinf(w[:, 0].astype(np.float32)))
    assert np.isnan(got[:, bad]).any() and not np.isnan(got[:, bad]).all()


# ---------------------------------------------------------------- refusals
def test_every_refusal_returns_err_arg_and_writes_nothing():
    T, N, C = 120, 5, 5
    bars = ohlcv(T, N, C)
    K = len(_names(FULL))

    def refused(**kw):
        rc, out = apply_raw(bars, kw.pop("spec", FULL), kw.pop("chan", CHANS[C]), rc_want=-1, **kw)
        assert np.all(out == SENTINEL)

    refused(T=L_FULL)                                                # T <= L
    refused(T=L_FULL - 3)
    refused(chan=(0, 1, 2, -1, 4))                                   # close is needed
    refused(chan=(0, 1, 2, 3, 5))                                    # volume >= C
    refused(chan=(0, -1, 2, 3, 4), spec=[("atr", {})])               # high is needed by atr
    refused(ldo=K + 1, col0=2)                                       # col0 + K > ldo
    refused(ldo=K - 1)
    refused(col0=-1, ldo=K + 2)
    refused(out_ptr=lambda bv: bv.data_ptr() + 4 * (bars.size - 1))  # out begins inside bars
    refused(out_ptr=lambda bv: bv.data_ptr())
    refused(work_short=8)                                            # a short workspace
    refused(work_off=4)                                              # a misaligned one
    apply_raw(bars, [("ema", {})], (-1, -1, -1, 3, -1))              # channels no op needs may be -1


# ---------------------------------------------------------------- hipGraph
@pytest.mark.parametrize("T", [400, L_FULL + 40])
def test_a_captured_call_replays_on_fresh_bars(T):
    from pmenv import _abi, features
    lib = _abi.load()
    N, C = 65, 5
    a, b = ohlcv(T, N, C), ohlcv(T, N, C, seed=1)
    ops, names = features.indicator_ops(FULL)
    K = len(names)
    bd = torch.from_numpy(a.copy()).to(DEV)
    out = torch.zeros(T - L_FULL, N, K, device=DEV)
    nbytes = lib.pmenv_ind_workspace(T, N, ops, len(ops))
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=DEV)
    chan = (ctypes.c_int32 * 5)(*CHANS[C])

    def call():
        rc = lib.pmenv_ind_apply(ctypes.c_void_p(bd.data_ptr()), T, N, C, chan, ops, len(ops),
                                 ctypes.c_void_p(out.data_ptr()), K, 0, ctypes.c_void_p(work.data_ptr()), nbytes,
                                 ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert rc == 0

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()                                                      # warm up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    eager = out.cpu().numpy().copy()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(eager))
    bd.copy_(torch.from_numpy(b.copy()))
    graph.replay()
    torch.cuda.synchronize(DEV)
    _, fresh = apply_raw(b, FULL, CHANS[C])
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(fresh))


# ---------------------------------------------------------------- build(indicators=...)
T_RAW, NB, CB = 330, 5, 5
SPEC_B = [("ema", {"timeperiod": 30}), ("bbands", {"timeperiod": 20}), ("macd", {}), ("rsi", {}), ("stoch", {}),
          ("obv", {})]


def _raw():
    bars = ohlcv(T_RAW, NB, CB, seed=3).copy()
    bars[..., 4] = np.float32(1.0) + bars[..., 4] / np.float32(2 ** 24)     # volumes of order 1
    return bars


def test_build_without_indicators_is_the_parent_pipeline():
    """the default leaves every byte as before: recomputed here from frac_diff and scale"""
    from pmenv import features
    raw = _raw()
    d = np.array([0.3, 0.5, 0.7, 0.4, 0.0])
    train, test = features.build(raw, d, thres=1e-2, scaler="minmax")
    assert not hasattr(train, "channel_names")
    r = torch.from_numpy(raw).to(DEV)
    x, widths, mw = features.frac_diff(r[1:].contiguous(), d, 1e-2)
    rel = (r[1:, :, 3] / r[:-1, :, 3])[mw:]
    n = x.shape[0]
    cut = int(0.8 * n)
    for part, lo, hi in ((train, 0, cut), (test, min(cut + mw, n), n)):
        y, _ = features.scale(x[lo:hi].contiguous(), "minmax")
        assert np.array_equal(_bits(part.bars.cpu().numpy()), _bits(y.cpu().numpy()))
        assert np.array_equal(_bits(part.relatives.cpu().numpy()), _bits(rel[lo:hi].cpu().numpy()))


def test_build_with_indicators_appends_clips_and_keeps_the_relatives_beside_their_rows():
    from pmenv import features
    raw = _raw()
    K, look, ind_names = features.indicator_layout(SPEC_B)
    assert (K, look) == (11, 33)
    train, test = features.build(raw, 0.0, scaler=None, indicators=SPEC_B, train_ratio=0.8,
                                 channel_names=["open", "high", "low", "close", "volume"])
    assert train.indicator_lookback == look and train.max_width == 0
    assert train.channel_names == ["open", "high", "low", "close", "volume"] + ind_names
    assert ind_names[:5] == ["ema_30", "upperband_20", "middleband_20", "lowerband_20", "macd_"]
    n = T_RAW - 1 - look
    assert train.days == int(0.8 * n) and test.days == n - int(0.8 * n)
    assert train.bars.shape == (train.days, NB, CB + K) and train.relatives.shape == (train.days, NB)
    got = np.concatenate([train.bars.cpu().numpy(), test.bars.cpu().numpy()])
    rel = np.concatenate([train.relatives.cpu().numpy(), test.relatives.cpu().numpy()])
    # d = 0, no scaler: the raw channels are rows 1 + look .. of raw, the relatives theirs
    assert np.array_equal(_bits(got[..., :CB]), _bits(raw[1 + look:]))
    # row i sits beside raw row 1 + look + i and keeps that row's relative, close[t] / close[t-1]
    close = torch.from_numpy(raw[..., 3].copy()).to(DEV)
    assert np.array_equal(_bits(rel), _bits((close[1 + look:] / close[look:-1]).cpu().numpy()))
    np.testing.assert_allclose(rel[1:], got[1:, :, 3] / got[:-1, :, 3], rtol=2.0 ** -23, atol=0)
    # the indicator channels are indicators() run alone on rows 1:
    cols, names, L = features.indicators(torch.from_numpy(raw[1:].copy()).to(DEV), SPEC_B)
    assert names == ind_names and L == look
    assert np.array_equal(_bits(got[..., CB:]), _bits(cols.cpu().numpy()))
    w, _ = ref.indicators(raw[1:], SPEC_B)
    check_values(got[..., CB:], w, ind_names)
    # d broadcasts over the C + K channels
    d = np.concatenate([[0.3, 0.5, 0.7, 0.4, 0.0], np.full(K, 0.2)])
    tr2, _ = features.build(raw, d, thres=1e-2, indicators=SPEC_B)
    assert tr2.widths.shape == (NB, CB + K) and tr2.max_width > 0 and int(tr2.widths[:, 4].max()) == 0
    assert tr2.bars.shape[2] == CB + K and tr2.relatives.shape[0] == tr2.days


def test_an_episode_runs_over_a_series_built_with_indicators():
    from pmenv import Episodes, TradingEnv, episodes, features, synth
    from pmenv.config import EnvConfig
    raw = _raw()
    train, _ = features.build(raw, 0.0, scaler="minmax", indicators=SPEC_B)
    B, W = 32, 8
    F = train.bars.shape[2] + 1
    cfg = EnvConfig(num_envs=B, num_assets=NB, window=W, features=F, close_channel=3)
    env = TradingEnv(config=cfg, device=DEV, track_info=False)
    rng = np.random.default_rng(3)
    length = rng.integers(10, 31, B)
    hi = train.days - W - 30
    assert hi > 20
    start, restart = rng.integers(0, hi, B), rng.integers(0, hi, B)
    ep = Episodes(train, W, start, restart=restart, length=length)
    obs = train.initial_window(ep.start, W)
    env.reset(obs)
    steps = int(length.max())
    act = synth.actions(steps, B, NB, seed=21, device=DEV)
    rewards, dones = episodes.collect(env, train, ep, obs, steps, act=act)
    assert torch.isfinite(rewards).all() and torch.isfinite(obs).all() and bool(dones.any())
