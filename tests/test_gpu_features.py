"""The feature pipeline on the GPU (pmenv.features; csrc/features.h): pmenv_ffd_apply bit for
bit against the numpy restatement of its contract (tests/ffd_ref.py) over the plan's edges,
its repeatability and NaN confinement, the column scalers against exactly summed
statistics, frac_diff / build against the reference's outputs (tests/golden/ffd/ffd_*.npz,
within the bounds test_features_host.py states), and a series with its own relatives
through episodes.collect and the compact rollout buffer. Needs an MI355X."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import ffd_ref
from episode_ref import restart_ref, window_ref
from ffd_ref import golden, golden_taps, table_of
from oracle import OracleEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KERNEL = "ffd_apply_kernel<8,8>"
CS = (1, 3, 63, 64, 65, 130)
MW = 66                                   # the widest filter of the raw-ABI cases: T = rows + 66 <= 400
SENTINEL = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    """bit-equal, any NaN standing for any NaN"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _placed(arr, off, dtype=torch.float32):
    """arr on the device `off` elements into a buffer of its own: (buffer, view)"""
    buf = torch.zeros(arr.size + off + 4, dtype=dtype, device=DEV)
    view = buf[off:off + arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr).ravel()))
    return buf, view


def _apply_raw(x, table, widths, mw, offs=(0, 0, 0)):
    """pmenv_ffd_apply through the raw ABI with x, the table and out at base offsets of
    offs floats; out sits between guard rows, which must come back untouched."""
    from pmenv import _abi
    lib = _abi.load()
    T, C = x.shape
    R = T - mw
    guard = 2 * C + 3
    _, xv = _placed(x, offs[0])
    _, tv = _placed(table if table.size else np.zeros(1, np.float32), offs[1])
    _, wv = _placed(widths, 0, torch.int32)
    ob = torch.full((guard + offs[2] + R * C + guard,), SENTINEL, device=DEV)
    ov = ob[guard + offs[2]:guard + offs[2] + R * C]
    rc = lib.pmenv_ffd_apply(ctypes.c_void_p(xv.data_ptr()), T, C, ctypes.c_void_p(tv.data_ptr()),
                             ctypes.c_void_p(wv.data_ptr()), mw, ctypes.c_void_p(ov.data_ptr()),
                             ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, rc
    full = ob.cpu().numpy()
    lo = guard + offs[2]
    assert np.all(full[:lo] == SENTINEL) and np.all(full[lo + R * C:] == SENTINEL), "guard rows written"
    return full[lo:lo + R * C].reshape(R, C)


def _plan(T, C, mw):
    from pmenv import features
    name, geo = features.ffd_path(T, C, mw)
    assert name == KERNEL, name                                   # the kernel by name before any value
    return geo


def _widths(C, mw, geo, shift):
    jb = geo["jb"]
    pool = [0, 1, 2, 7, 8, 9, 63, 64, 65, mw, jb - 1, jb, jb + 1]
    return np.array([pool[(c + shift) % len(pool)] for c in range(C)], dtype=np.int32)


def _case(T, C, mw, seed, shift=0):
    """(x, table, widths): arbitrary taps (widths need no real d), NaN in every table row a
    column's width excludes — the kernel must not use them"""
    rng = np.random.default_rng(seed)
    geo = _plan(T, C, mw)
    widths = _widths(C, mw, geo, shift)
    x = (rng.normal(size=(T, C)) * np.exp(rng.normal(size=(1, C)) * 3)).astype(np.float32)
    table = rng.normal(size=(mw, C)).astype(np.float32)
    for c in range(C):
        table[widths[c]:, c] = np.nan
    return x, table, widths


def _row_counts(C):
    geo = _plan(MW + 64, C, MW)
    chunk = geo["slots"] * geo["rb"]                              # a wave's time chunk
    out = {1, 63, 64, 65, 257}
    for size in (geo["rows"], geo["rb"], chunk):
        out |= {size - 1, size, size + 1}
    return sorted(r for r in out if r >= 1)


@pytest.mark.parametrize("C", CS)
def test_ffd_apply_equals_the_restatement_bit_for_bit(C):
    """every output-row count one each side of the plan's register block, wave chunk and
    workgroup chunk, widths mixed inside a wave one each side of the tap block, base offsets of
    0 .. 3 floats on x, the table and out"""
    for i, R in enumerate(_row_counts(C)):
        T = R + MW
        assert T <= 400
        geo = _plan(T, C, MW)
        assert geo["grid"] == (-(-R // geo["rows"]), -(-C // geo["cw"]))
        x, table, widths = _case(T, C, MW, seed=1000 * C + R, shift=i)
        offs = (i % 4, (i // 2) % 4, (i + 3) % 4)
        got = _apply_raw(x, table, widths, MW, offs)
        want = ffd_ref.ffd_ref(x, np.nan_to_num(table), widths, MW)
        assert np.isfinite(want).all()
        assert np.array_equal(_bits(got), _bits(want)), (C, R, offs, np.argwhere(_bits(got) != _bits(want))[:4])


def test_ffd_apply_single_column_every_width():
    """C = 1 holds one width per call: each of them in turn, and max_width beyond every width"""
    geo = _plan(100 + MW, 1, MW)
    for shift in range(13):
        x, table, widths = _case(100 + MW, 1, MW, seed=shift, shift=shift)
        got = _apply_raw(x, table, widths, MW, (shift % 4, 0, 0))
        assert np.array_equal(_bits(got), _bits(ffd_ref.ffd_ref(x, np.nan_to_num(table), widths, MW))), widths
    assert geo["cw"] == 16
    x = np.arange(12, dtype=np.float32).reshape(12, 1)
    got = _apply_raw(x, np.zeros((0, 1), np.float32), np.zeros(1, np.int32), 0)   # no filter at all: a copy
    assert np.array_equal(got, x)


def test_ffd_apply_repeats_and_replays_from_a_captured_graph():
    from pmenv import features
    T, C = 257 + MW, 130
    x, table, widths = _case(T, C, MW, seed=77)
    x2 = np.random.default_rng(78).normal(size=(T, C)).astype(np.float32)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(np.nan_to_num(table)).to(DEV)
    wd = torch.from_numpy(widths).to(DEV)
    first = features.ffd_apply(xd, td, wd, MW).cpu().numpy()
    again = features.ffd_apply(xd, td, wd, MW).cpu().numpy()
    assert np.array_equal(_bits(first), _bits(again))
    out = torch.zeros(T - MW, C, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        features.ffd_apply(xd, td, wd, MW, out=out)               # warm up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        features.ffd_apply(xd, td, wd, MW, out=out)
    graph.replay()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(first))
    xd.copy_(torch.from_numpy(x2))                                # fresh x under the same graph
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ffd_ref.ffd_ref(x2, np.nan_to_num(table), widths, MW)))


def test_ffd_apply_confines_a_nan_to_its_column_and_width():
    T, C = 150 + MW, 65
    x, table, widths = _case(T, C, MW, seed=5)
    base = _apply_raw(x, table, widths, MW)
    for c0, t0 in ((0, 100), (3, MW + 5), (9, 80), (8, T - 3), (12, 120), (64, 10), (7, 90)):
        y = x.copy()
        y[t0, c0] = np.nan
        got = _apply_raw(y, table, widths, MW)
        w = int(widths[c0])
        rows = [t - MW for t in range(t0, t0 + max(w, 1)) if MW <= t < T]     # width 0 copies x[t]: one row
        nan = np.zeros_like(got, dtype=bool)
        nan[rows, c0] = True
        assert np.array_equal(np.isnan(got), nan), (c0, t0, w)
        assert np.array_equal(_bits(got)[~nan], _bits(base)[~nan])            # every other element: the same bits


# ---------------------------------------------------------------- the scalers
def _scale_input(T, C, seed):
    """columns by kind, c % 5: random about 3; constant; one NaN; 1,000 +- 0.25; zeros of both signs"""
    rng = np.random.default_rng(seed)
    x = np.empty((T, C), dtype=np.float32)
    for c in range(C):
        kind = (c + seed) % 5
        if kind == 0:
            x[:, c] = 3.0 + rng.normal(size=T)
        elif kind == 1:
            x[:, c] = np.float32(0.1) if c % 2 else 3.5
        elif kind == 2:
            x[:, c] = 5.0 + rng.normal(size=T)
            x[rng.integers(T), c] = np.nan
        elif kind == 3:
            x[:, c] = 1000.0 + 0.25 * rng.choice([-1.0, 0.0, 1.0], size=T)
        else:
            x[:, c] = np.where(rng.random(T) < 0.5, -0.0, 0.0)       # a few positive values: a mean that is no cancellation
            some = rng.random(T) < 0.2
            x[some, c] = np.abs(rng.normal(size=T))[some]
    return x


def _ulp_close(got, want):
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    g, w = got[~nan].astype(np.float64), want[~nan].astype(np.float64)
    return bool(np.all(np.abs(g - w) <= np.spacing(np.abs(want[~nan]).astype(np.float32))))


@pytest.mark.parametrize("method", ["minmax", "standard"])
@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 1000])
def test_scalers_against_exactly_summed_statistics(T, method):
    from pmenv import features
    for C in CS:
        x = _scale_input(T, C, seed=T + C)
        xd = torch.from_numpy(x).to(DEV)
        y, stats = features.scale(xd, method)
        want_y, want = ffd_ref.scale_ref(x, method)
        st = stats.cpu().numpy()
        assert st.shape == (2, C) and stats.dtype == torch.float64
        assert np.array_equal(np.isnan(st), np.isnan(want)), (T, C)
        ok = ~np.isnan(want)
        if method == "minmax":
            assert np.array_equal(st[ok], want[ok]), (T, C)                   # min / max exact
        else:
            assert np.all(np.abs(st[0][ok[0]] - want[0][ok[0]]) <= 1e-12 * np.abs(want[0][ok[0]])), (T, C)
            assert np.all(np.abs(st[1][ok[1]] - want[1][ok[1]]) <= 1e-12 * np.abs(want[1][ok[1]])), (T, C)
        got = y.cpu().numpy()
        assert _ulp_close(got, want_y), (T, C, method)
        z = xd.clone()
        z2, _ = features.scale(z, method, stats=stats, out=z)                 # in place, the fit's stats given
        assert z2.data_ptr() == z.data_ptr() and _same(z.cpu().numpy(), got)
        assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x))              # out of place left x alone
        # another fit's statistics are honoured: these rows by the statistics of x
        x2 = _scale_input(T, C, seed=T + C + 1)
        y2, st2 = features.scale(torch.from_numpy(x2).to(DEV), method, stats=stats)
        assert st2 is stats
        assert _ulp_close(y2.cpu().numpy(), ffd_ref.scale_ref(x2, method, stats=st)[0]), (T, C)


def test_scalers_confine_an_inf_to_its_column():
    from pmenv import features
    x = _scale_input(300, 65, seed=4)
    base = {m: features.scale(torch.from_numpy(x).to(DEV), m)[0].cpu().numpy() for m in ("minmax", "standard")}
    x[17, 20] = np.inf
    for m in ("minmax", "standard"):
        got = features.scale(torch.from_numpy(x).to(DEV), m)[0].cpu().numpy()
        others = np.ones(65, bool)
        others[20] = False
        assert _same(got[:, others], base[m][:, others]) and not np.isfinite(got[17, 20])


# ---------------------------------------------------------------- the goldens
@functools.lru_cache(maxsize=None)
def _golden_run(name):
    """frac_diff on a golden's features: (golden, out, widths, max_width, table)"""
    from pmenv import features
    g = golden(name)
    x = g["raw"][1:]
    out, widths, mw = features.frac_diff(torch.from_numpy(x).to(DEV), g["d"], float(g["thres"]))
    return g, out.cpu().numpy(), widths.cpu().numpy(), mw, table_of(golden_taps(g))[0]


@pytest.mark.parametrize("name", ["mixed_t600", "t6000"])
def test_frac_diff_reproduces_the_reference_transform(name):
    g, out, widths, mw, table = _golden_run(name)
    x = g["raw"][1:]
    _plan(x.shape[0], x.shape[1], mw)
    assert mw == int(g["max_width"]) and np.array_equal(widths, g["widths"])
    assert np.array_equal(_bits(out), _bits(ffd_ref.ffd_ref(x, table, widths, mw)))          # the contract
    err = np.abs(out.astype(np.float64) - g["ffd"].astype(np.float64))
    bound = ffd_ref.ffd_bound(x, table, widths, mw, g["ffd"])
    print(f"{name}: largest error / bound = {(err / bound).max():.3g}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("method", ["minmax", "standard"])
def test_scalers_reproduce_sklearn_on_the_reference_rows(method):
    from pmenv import features
    g = golden("mixed_t600")
    split, purge = int(g["split"]), int(g["purge"])
    for part, rows in (("train", g["ffd"][:split]), ("test", g["ffd"][split + purge:])):
        y, stats = features.scale(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), method)
        y, st = y.cpu().numpy(), stats.cpu().numpy()
        err = np.abs(y.astype(np.float64) - g[f"{part}_{method}"].astype(np.float64))
        bound = ffd_ref.scale_bound(rows, y, st, method)
        print(f"{method} {part}: largest error / bound = {(err / bound).max():.3g}")
        assert np.all(err <= bound)


@pytest.mark.parametrize("scaler", ["minmax", "standard", None])
def test_build_follows_the_loader_order_on_the_golden(scaler):
    """One ticker through build(): the row counts of the reference's split and purge, the
    relatives clipped with the features, and the parts against sklearn's. The parts here are
    scaled from this library's FFD rows, sklearn's from the reference's: an FFD difference of
    at most e in a column moves x, min / mean and max / std by e each, so y by at most
    (2 + 2 |y|) e / (range or std) on top of the scaler bound."""
    from pmenv import features
    g, out, widths, mw, table = _golden_run("mixed_t600")
    raw = g["raw"][:, None, :]
    train, test = features.build(raw, g["d"], thres=float(g["thres"]), train_ratio=0.8, scaler=scaler,
                                 close_channel=list(g["names"]).index("close"))
    n = raw.shape[0] - 1 - mw
    split = int(0.8 * n)
    assert split == int(g["split"]) and mw == int(g["purge"]) == train.max_width == test.max_width
    assert train.bars.shape == (split, 1, raw.shape[2]) and test.bars.shape == (n - split - mw, 1, raw.shape[2])
    assert train.relatives.shape == (split, 1) and test.relatives.shape == (n - split - mw, 1)
    assert np.array_equal(train.widths.cpu().numpy(), g["widths"][None, :])
    rel = g["relatives"][mw:]
    np.testing.assert_allclose(train.relatives.cpu().numpy()[:, 0], rel[:split], rtol=2.0 ** -23, atol=0)
    np.testing.assert_allclose(test.relatives.cpu().numpy()[:, 0], rel[split + mw:], rtol=2.0 ** -23, atol=0)
    e = np.abs(out.astype(np.float64) - g["ffd"].astype(np.float64)).max(axis=0)
    for part, series, rows in (("train", train, out[:split]), ("test", test, out[split + mw:])):
        got = series.bars.cpu().numpy()[:, 0, :]
        if scaler is None:
            assert np.array_equal(_bits(got), _bits(rows))
            continue
        y, st = ffd_ref.scale_ref(rows, scaler)
        assert _ulp_close(got, y)
        den = st[1] if scaler == "standard" else st[1] - st[0]
        den = np.where(den == 0.0, 1.0, den)
        bound = ffd_ref.scale_bound(rows, got, st, scaler) + (2 + 2 * np.abs(got)) * e[None, :] / den[None, :]
        assert np.all(np.abs(got.astype(np.float64) - g[f"{part}_{scaler}"]) <= bound)


# ---------------------------------------------------------------- end to end
T_RAW = 300
B, N, W, C = 96, 5, 8, 5                  # F = 6: the tiny step and the generic two-launch stream
F = C + 1
WIDE = (64, 30, 50, 4)                    # F = 5: the one-launch steps (flat, relay, one workgroup per env) as well


@functools.lru_cache(maxsize=None)
def _built(N=N, C=C):
    from pmenv import features
    rng = np.random.default_rng(12)
    close = 50 * np.exp(np.cumsum(0.012 * rng.standard_normal((T_RAW, N)), axis=0))
    raw = np.empty((T_RAW, N, C), np.float32)
    for c in range(C):
        raw[..., c] = close * np.exp(0.003 * rng.standard_normal(close.shape))
    raw[..., 3] = close
    d = np.array([0.3, 0.5, 0.7, 0.4, 0.0])[:C]
    train, test = features.build(raw, d, thres=1e-2, train_ratio=0.8, scaler="minmax", close_channel=3)
    return raw, train, test


def _episode_setup(train, B=B, W=W):
    rng = np.random.default_rng(3)
    length = rng.integers(10, 31, B)
    hi = train.days - W - 30
    assert hi > 20
    start, restart = rng.integers(0, hi, B), rng.integers(0, hi, B)
    return start, restart, length


def _impls(B=B, N=N, W=W, F=F):
    from pmenv import step_path_for
    return [i for i in ("auto", "one_launch", "two_launch", "flat", "relay")
            if step_path_for(num_envs=B, num_assets=N, window=W, features=F, step_impl=i, close_channel=3) != ""]


def _env(impl, B=B, N=N, W=W, F=F):
    from pmenv import TradingEnv
    from pmenv.config import EnvConfig
    cfg = EnvConfig(num_envs=B, num_assets=N, window=W, features=F, close_channel=3)
    env = TradingEnv(config=cfg, device=DEV, track_info=False)
    env.set_step_impl(impl)
    return env, cfg


def test_built_series_is_what_the_loader_order_gives():
    raw, train, test = _built()
    mw = train.max_width
    n = T_RAW - 1 - mw
    assert mw > 0 and train.days == int(0.8 * n) and test.days == n - int(0.8 * n) - mw
    assert train.relatives.shape == (train.days, N) and train.bars.shape == (train.days, N, C)
    rel = raw[1:, :, 3] / raw[:-1, :, 3]
    np.testing.assert_allclose(train.relatives.cpu().numpy(), rel[mw:mw + train.days], rtol=2.0 ** -23, atol=0)
    bars = train.bars.cpu().numpy()
    assert bars.min() == 0.0 and bars.max() == 1.0                            # min-max scaled per column
    assert train.widths.shape == (N, C) and int(train.widths[:, 4].max()) == 0


@pytest.mark.parametrize("shape", [(B, N, W, C), WIDE], ids=lambda s: "x".join(map(str, s)))
def test_collect_on_a_built_series_uses_its_relatives(shape):
    """episodes.collect on features.build's train part, on every step path the shape admits:
    the rewards against the CPU checker fed the same windows and prices = relatives[day]
    (the tolerances of the other parity tests); the same bars without the table give other
    rewards: the table is what the step used."""
    from pmenv import Episodes, MarketSeries, episodes, synth
    B, N, W, C = shape
    F = C + 1
    raw, train, _ = _built(N, C)
    bars, rel = train.bars.cpu().numpy(), train.relatives.cpu().numpy()
    start, restart, length = _episode_setup(train, B, W)
    steps = 3 * int(length.max())
    act = synth.actions(steps, B, N, seed=21, device=DEV)
    act_h = act.cpu().numpy()
    impls = _impls(B, N, W, F)
    assert "auto" in impls and "two_launch" in impls and (F != 5 or {"flat", "relay", "one_launch"} <= set(impls))
    runs = {}
    for impl in impls:
        env, cfg = _env(impl, B, N, W, F)
        ep = Episodes(train, W, start, restart=restart, length=length)
        obs = train.initial_window(ep.start, W)
        env.reset(obs)
        rewards, dones = episodes.collect(env, train, ep, obs, steps, act=act)
        runs[impl] = (rewards.cpu().numpy(), dones.cpu().numpy(), env.step_path)
    g_r, g_d, _ = runs["auto"]
    cenv = OracleEnv(cfg)
    cobs = window_ref(bars, start, W, F)
    cenv.reset(cobs)
    day, end = start + W, start + W + length
    for t in range(steps):
        cr, _, _ = cenv.step(act_h[t], cobs, prices=rel[day], bar=bars[day])
        for impl in impls:
            err = np.abs(runs[impl][0][t].astype(np.float64) - cr)
            assert np.all(err <= 1e-6 * np.abs(cr) + 1e-9), f"{impl} step {t}: reward err {err.max():.3e}"
        done, day = restart_ref(day, end, restart, W)
        for impl in impls:
            assert np.array_equal(runs[impl][1][t], done), (impl, t)
        if done.any():
            cobs[done] = window_ref(bars, restart[done], W, F)
            cenv.reset(cobs, mask=done)
            end = np.where(done, restart + W + length, end)
    assert g_d.sum(0).min() >= 2 and np.isfinite(g_r).all()
    # the same bars as a plain series: p = scaled close / scaled close
    plain = MarketSeries(train.bars)
    env, _ = _env("auto", B, N, W, F)
    ep = Episodes(plain, W, start, restart=restart, length=length)
    obs = plain.initial_window(ep.start, W)
    env.reset(obs)
    p_r = episodes.collect(env, plain, ep, obs, steps, act=act)[0].cpu().numpy()
    differs = ~np.isfinite(p_r) | (p_r != g_r)
    assert differs.mean() > 0.9


def test_compact_rollout_buffer_reads_p_from_the_table():
    """DeviceRolloutBuffer(episodes=True) over the same run: price_relatives(t) and gather's p
    bit-equal to relatives[day of the step], and the recorded rewards those of collect."""
    from pmenv import DeviceRolloutBuffer, Episodes, episodes, synth
    raw, train, _ = _built()
    rel = train.relatives
    start, restart, length = _episode_setup(train)
    steps = 3 * int(length.max())
    act = synth.actions(steps, B, N, seed=21, device=DEV)
    env, _ = _env("auto")
    ep = Episodes(train, W, start, restart=restart, length=length)
    obs = train.initial_window(ep.start, W)
    env.reset(obs)
    buf = DeviceRolloutBuffer(B, N, W, steps, features=F, device=DEV, close_channel=3, series=train, episodes=True)
    buf.reset(start=ep.start)
    w = torch.empty(B, N, device=DEV)
    days = torch.empty(steps + 1, B, dtype=torch.long, device=DEV)
    for t in range(1, steps + 1):
        days[t] = ep.next_day
        r, _ = env.step(act[t - 1], obs, series=train, day=ep.next_day, weights_out=w)
        buf.add(act[t - 1], env.value, r, weights=w)
        buf.restarted(env.restart(obs, ep), ep.next_day)
    env2, _ = _env("auto")
    ep2 = Episodes(train, W, start, restart=restart, length=length)
    obs2 = train.initial_window(ep2.start, W)
    env2.reset(obs2)
    want_r = episodes.collect(env2, train, ep2, obs2, steps, act=act)[0]
    assert torch.equal(buf.r[1:], want_r)
    for t in (1, 2, int(length.min()), int(length.min()) + 1, steps // 2, steps):
        assert torch.equal(buf.price_relatives(t), rel[days[t]]), t
    g = torch.Generator().manual_seed(5)
    tt = torch.randint(1, steps + 1, (257,), generator=g).to(DEV)
    ee = torch.randint(0, B, (257,), generator=g).to(DEV)
    s, a, r, v_prev, a_prev, p = buf.gather(tt, ee)
    assert p.shape == (257, N, 1) and torch.equal(p[..., 0], rel[days[tt, ee], :])
    assert s.shape == (257, N, W, F)


def test_plain_series_steps_as_the_bar_path_does():
    """A MarketSeries without a table is untouched by all this: its step is bit-equal to the
    step fed the same day's bars with prices=None."""
    from pmenv import MarketSeries, synth
    raw, _, _ = _built()
    ms = MarketSeries(raw)
    assert ms.relatives is None
    act = synth.actions(12, B, N, seed=2, device=DEV)
    start = torch.arange(B, dtype=torch.int32, device=DEV) % 40
    outs = []
    for mode in ("series", "bar"):
        env, _ = _env("auto")
        obs = ms.initial_window(start, W)
        env.reset(obs)
        rs = []
        for t in range(12):
            day = start + W + t
            if mode == "series":
                r, _ = env.step(act[t], obs, series=ms, day=day)
            else:
                r, _ = env.step(act[t], obs, prices=None, bar=ms.bars[day.long()].contiguous())
            rs.append(r.clone())
        outs.append((torch.stack(rs), obs.clone(), env.value.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert math.isfinite(float(outs[0][0].sum()))
