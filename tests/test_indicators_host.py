"""The technical indicators on the CPU. The numpy restatement of their definitions
(tests/indicators_ref.py, what the GPU tests compare the kernels with) is checked against
closed forms, so that it is not its own oracle. Then, through the library without a device:
pmenv_ind_layout's lookbacks and output counts, the refusals, pmenv_ind_path's form rule and
geometry against a Python transcription over a sweep of T and N either side of its
thresholds, and the output names against the reference's rule (instrument.py:227-229).
tests/host/ind_plan_sweep.cpp, a program that includes nothing but csrc/ind_plan.h, is
compiled with the plain host C++ compiler — and once more under the address and
undefined-behaviour sanitizers, run as its own process — and must print what the library
returns."""
import ctypes
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import indicators_ref as ref
from pmenv import _abi, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_SRC = os.path.join(ROOT, "tests", "host", "ind_plan_sweep.cpp")
SPLIT_MAX_COLS, SEG_ROWS, MAX_SEGS, SLOTS, BLOCK = 16384, 32, 64, 18, 256
I32_MAX = 2 ** 31 - 1
T0 = 200


def ramp(T=T0):
    return np.arange(T, dtype=np.float64)[:, None]


# ---------------------------------------------------------------- the restatement against closed forms
@pytest.mark.parametrize("p", [2, 5, 14, 30])
def test_ema_of_a_ramp_lags_by_half_the_period(p):
    got = ref.ema(ramp(), p)[:, 0, 0]
    t = np.arange(p - 1, T0)
    np.testing.assert_allclose(got, t - (p - 1) / 2, rtol=0, atol=1e-10)


@pytest.mark.parametrize("fast,slow,signal", [(12, 26, 9), (2, 5, 2), (14, 5, 30)])
def test_macd_of_a_ramp_is_half_the_period_difference(fast, slow, signal):
    got = ref.macd(ramp(), fast, slow, signal)[:, 0]
    assert got.shape[0] == T0 - ref.lookback("macd", dict(fastperiod=fast, slowperiod=slow, signalperiod=signal))
    np.testing.assert_allclose(got[:, 0], abs(slow - fast) / 2, rtol=0, atol=1e-10)
    np.testing.assert_allclose(got[:, 1], abs(slow - fast) / 2, rtol=0, atol=1e-10)
    np.testing.assert_allclose(got[:, 2], 0.0, rtol=0, atol=1e-10)


def test_constant_series():
    c = np.full((T0, 1), 42.5)
    bands = ref.bbands(c, 20, 2.0, 2.0)
    assert np.all(bands == 42.5)                                      # three equal bands: var is 0 or below
    assert np.all(ref.ema(c, 30) == 42.5)
    assert np.all(ref.cci(c, c, c, 14) == 0.0)
    assert np.all(ref.stoch(c, c, c, 5, 3, 3) == 0.0)


@pytest.mark.parametrize("p", [2, 14])
def test_rsi_of_monotone_closes(p):
    rng = np.random.default_rng(0)
    up = np.cumsum(rng.uniform(0.1, 1.0, (T0, 1)), axis=0)
    assert np.all(ref.rsi(up, p) == 100.0)
    assert np.all(ref.rsi(-up, p) == 0.0)
    assert np.all(ref.rsi(np.full((T0, 1), 3.0), p) == 0.0)           # no movement at all: the guarded 0


@pytest.mark.parametrize("p", [2, 14])
def test_atr_of_bars_of_constant_range(p):
    rng = np.random.default_rng(1)
    mid = 100.0 + np.cumsum(rng.uniform(-0.2, 0.2, (T0, 1)), axis=0)   # moves less than the half range
    r = 4.0
    h, l = mid + r / 2, mid - r / 2
    c = mid + rng.uniform(-0.5, 0.5, (T0, 1))
    np.testing.assert_allclose(ref.atr(h, l, c, p), r, rtol=1e-12, atol=0)


@pytest.mark.parametrize("p", [2, 5, 14])
def test_dx_and_adx_of_a_steady_up_trend(p):
    t = ramp(120)
    h, l, c = 10.0 + t + 1.0, 10.0 + t - 1.0, 10.0 + t
    plus, minus = ref.directional_movement(h, l)
    assert np.all(plus > 0) and np.all(minus == 0)
    np.testing.assert_allclose(ref.dx(h, l, c, p), 100.0, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref.adx(h, l, c, p), 100.0, rtol=1e-12, atol=0)
    flat = np.full((120, 1), 5.0)                                     # deviation 1: a flat series gives 0
    assert np.all(ref.dx(flat, flat, flat, p) == 0.0) and np.all(ref.adx(flat, flat, flat, p) == 0.0)


def test_obv_of_a_rising_close_is_the_cumulative_volume():
    rng = np.random.default_rng(2)
    v = rng.integers(1, 2 ** 24, (T0, 3)).astype(np.float64)
    c = np.cumsum(rng.uniform(0.1, 1.0, (T0, 3)), axis=0)
    assert np.array_equal(ref.obv(c, v)[..., 0], np.cumsum(v, axis=0))
    assert np.array_equal(ref.obv(-c, v)[1:, :, 0], v[0] - np.cumsum(v[1:], axis=0))


def test_adosc_is_zero_while_the_close_is_the_midpoint():
    rng = np.random.default_rng(3)
    c = 50.0 + np.cumsum(rng.standard_normal((T0, 2)), axis=0)
    half = rng.integers(1, 9, (T0, 2)) / 8.0                          # exact in binary: c is the midpoint exactly
    v = rng.integers(1, 2 ** 24, (T0, 2)).astype(np.float64)
    assert np.all(ref.adosc(c + half, c - half, c, v, 3, 10) == 0.0)


def test_windowed_values_against_direct_numpy():
    rng = np.random.default_rng(4)
    c = 50.0 + np.cumsum(rng.standard_normal((T0, 2)), axis=0)
    h, l = c + rng.uniform(0, 1, c.shape), c - rng.uniform(0, 1, c.shape)
    p = 14
    win = np.lib.stride_tricks.sliding_window_view(c, p, axis=0)       # [T - p + 1, 2, p]
    b = ref.bbands(c, p, 2.0, 1.0)
    np.testing.assert_allclose(b[..., 1], win.mean(-1), rtol=1e-13)
    np.testing.assert_allclose(b[..., 0] - b[..., 1], 2.0 * win.std(-1), rtol=1e-7)
    np.testing.assert_allclose(b[..., 1] - b[..., 2], win.std(-1), rtol=1e-7)
    tp = np.lib.stride_tricks.sliding_window_view((h + l + c) / 3.0, p, axis=0)
    md = np.abs(tp - tp.mean(-1, keepdims=True)).mean(-1)
    np.testing.assert_allclose(ref.cci(h, l, c, p)[..., 0], (tp[..., -1] - tp.mean(-1)) / (0.015 * md), rtol=1e-9)
    hh = np.lib.stride_tricks.sliding_window_view(h, 5, axis=0).max(-1)
    ll = np.lib.stride_tricks.sliding_window_view(l, 5, axis=0).min(-1)
    fastk = 100.0 * (c[4:] - ll) / (hh - ll)
    slowk = np.lib.stride_tricks.sliding_window_view(fastk, 3, axis=0).mean(-1)
    slowd = np.lib.stride_tricks.sliding_window_view(slowk, 3, axis=0).mean(-1)
    s = ref.stoch(h, l, c, 5, 3, 3)
    np.testing.assert_allclose(s[..., 0], slowk[2:], rtol=1e-12)
    np.testing.assert_allclose(s[..., 1], slowd, rtol=1e-12)


# ---------------------------------------------------------------- pmenv_ind_layout
SINGLE = [("ema", {"timeperiod": 30}), ("ema", {"timeperiod": 2}), ("bbands", {"timeperiod": 20}), ("macd", {}),
          ("macd", {"fastperiod": 26, "slowperiod": 12, "signalperiod": 2}), ("atr", {}), ("rsi", {"timeperiod": 30}),
          ("adx", {"timeperiod": 30}), ("dx", {"timeperiod": 30}), ("stoch", {}),
          ("stoch", {"fastk_period": 14, "slowk_period": 5, "slowd_period": 2}), ("cci", {}), ("obv", {}), ("adosc", {}),
          ("adosc", {"fastperiod": 14, "slowperiod": 5}), ("ema", {"timeperiod": 256})]


def test_layout_gives_every_ops_lookback_and_output_count():
    for name, params in SINGLE:
        K, L, names = features.indicator_layout([(name, params)])
        assert (K, L) == (ref.OUTPUTS[name], ref.lookback(name, params)), (name, params)
        assert len(names) == K
    defaults = {n: features.indicator_layout([(n, {})])[1] for n in ref.DEFAULTS}
    assert defaults == dict(ema=29, bbands=4, macd=33, atr=14, rsi=14, adx=27, dx=14, stoch=8, cci=13, obv=0, adosc=9)


def test_lookbacks_are_additive_and_a_call_takes_the_largest():
    for fk, sk, sd in itertools.product((2, 5, 14), repeat=3):
        p = dict(fastk_period=fk, slowk_period=sk, slowd_period=sd)
        assert features.indicator_layout([("stoch", p)])[1] == (fk - 1) + (sk - 1) + (sd - 1)
    for slow, sig in itertools.product((5, 26, 256), (2, 9, 256)):
        p = dict(fastperiod=3, slowperiod=slow, signalperiod=sig)
        assert features.indicator_layout([("macd", p)])[1] == (slow - 1) + (sig - 1)
    for p in (2, 14, 256):
        assert features.indicator_layout([("adx", {"timeperiod": p})])[1] == \
            features.indicator_layout([("dx", {"timeperiod": p})])[1] + (p - 1)
    K, L, _ = features.indicator_layout(SINGLE)
    assert K == sum(ref.OUTPUTS[n] for n, _ in SINGLE) and L == max(ref.lookback(n, p) for n, p in SINGLE) == 255


def _op(kind, p=(14, 14, 14), f=(2.0, 2.0)):
    op = _abi.PmenvIndOp()
    op.kind = kind
    op.p[:] = p
    op.f[:] = f
    return op


def test_every_out_of_range_parameter_is_refused():
    lib = _abi.load()
    K, L = ctypes.c_int32(7), ctypes.c_int32(7)

    def rc(*ops, n=None):
        arr = (_abi.PmenvIndOp * max(len(ops), 1))(*ops)
        return lib.pmenv_ind_layout(arr, len(ops) if n is None else n, ctypes.byref(K), ctypes.byref(L))

    used = {0: 1, 1: 1, 2: 3, 3: 1, 4: 1, 5: 1, 6: 1, 7: 3, 8: 1, 9: 0, 10: 2}    # period arguments per kind
    for kind, n_p in used.items():
        assert rc(_op(kind)) == 0, kind
        for i in range(3):
            for bad in (1, 0, -5, 257, I32_MAX, -I32_MAX - 1):
                p = [14, 14, 14]
                p[i] = bad
                assert rc(_op(kind, p)) == (-1 if i < n_p else 0), (kind, i, bad)
            for good in (2, 256):
                p = [14, 14, 14]
                p[i] = good
                assert rc(_op(kind, p)) == 0, (kind, i, good)
    for kind in (-1, 11, 100, I32_MAX):
        assert rc(_op(kind)) == -1
    for f in ((float("nan"), 2.0), (2.0, float("inf")), (-float("inf"), 2.0)):
        assert rc(_op(1, f=f)) == -1 and rc(_op(0, f=f)) == 0             # the multipliers are bbands' alone
    assert rc(_op(0), _op(11)) == -1                                      # one bad op refuses the call
    assert rc(n=0) == -1 and rc(_op(0), n=-1) == -1
    assert rc(*[_op(0)] * 32) == 0 and rc(*[_op(0)] * 33) == -1
    assert lib.pmenv_ind_layout(None, 1, ctypes.byref(K), ctypes.byref(L)) == -1
    one = (_abi.PmenvIndOp * 1)(_op(5))
    assert lib.pmenv_ind_layout(one, 1, None, None) == 0                  # either output may be NULL
    assert lib.pmenv_ind_workspace(27, 4, one, 1) == 0 and lib.pmenv_ind_path(27, 4, one, 1) == b""   # T <= L
    assert lib.pmenv_ind_path(28, 0, one, 1) == b"" and lib.pmenv_ind_path(28, 4, one, 1) != b""


def test_python_refuses_what_the_reference_could_not_mean():
    for spec in ([("sma", {})], [("ema", {"period": 3})], [("bbands", {"matype": 1})], [("stoch", {"slowk_matype": 2})],
                 [("stoch", {"slowd_matype": 1})], [("ema", {"timeperiod": 2.5})], []):
        with pytest.raises(ValueError):
            features.indicator_ops(spec)
    with pytest.raises(_abi.PmenvError):
        features.indicator_layout([("ema", {"timeperiod": 1})])
    features.indicator_ops([("bbands", {"matype": 0}), ("stoch", {"slowk_matype": 0, "slowd_matype": 0})])


def test_names_follow_the_reference_rule():
    """instrument.py:227-229: `real` takes the indicator's name; "_" + the given values joined by "_" """
    spec = [("EMA", {"timeperiod": 30}), ("ema", {"timeperiod": 60}), ("bbands", {"timeperiod": 20}), ("macd", {}),
            ("atr", {}), ("Rsi", {"timeperiod": 30}), ("stoch", {}), ("obv", {}),
            ("bbands", {"timeperiod": 5, "nbdevup": 2.5, "nbdevdn": 1}), ("adosc", {"fastperiod": 3, "slowperiod": 10})]
    want = []
    outputs = dict(ema=["real"], bbands=["upperband", "middleband", "lowerband"], macd=["macd", "macdsignal", "macdhist"],
                   atr=["real"], rsi=["real"], stoch=["slowk", "slowd"], obv=["real"], adosc=["real"])
    for indicator, params in spec:
        indicator = indicator.lower()
        for name in outputs[indicator]:
            if name == 'real': name = indicator                             # noqa: E701 (the reference's lines)
            want.append(name + '_' + '_'.join([f'{value}' for value in params.values()]))
    _, _, names = features.indicator_layout(spec)
    assert names == want
    assert names[:5] == ["ema_30", "ema_60", "upperband_20", "middleband_20", "lowerband_20"]
    assert names[5:8] == ["macd_", "macdsignal_", "macdhist_"] and names[-4:-1] == ["upperband_5_2.5_1"] + \
        ["middleband_5_2.5_1", "lowerband_5_2.5_1"] and names[-1] == "adosc_3_10"


# ---------------------------------------------------------------- the plan, transcribed
SCAN = {"ema", "macd", "atr", "rsi", "adx", "dx", "obv", "adosc"}


def expected_path(T, N, spec):
    try:
        K, L, _ = features.indicator_layout(spec)
    except _abi.PmenvError:
        return "", 0
    if N < 1 or T <= L:
        return "", 0
    R = T - L
    count = {}
    for name, _ in spec:
        if name in SCAN:
            count[name] = count.get(name, 0) + 1
    walks = max(count.values(), default=0)
    n_window = sum(name not in SCAN for name, _ in spec)
    stoch = any(name == "stoch" for name, _ in spec)
    sg, wg, fg = -(-N // 64), -(-R * N // BLOCK), -(-T * N // BLOCK)
    if max(sg, wg, fg) > I32_MAX:
        return "", 0
    parts, rec = [], 0
    if walks:
        if N <= SPLIT_MAX_COLS and R >= 2 * SEG_ROWS:
            seg = max(SEG_ROWS, -(-R // MAX_SEGS))
            segs = -(-R // seg)
            parts.append(f"ind_scan_split_kernel walks={walks} seg={seg} segs={segs} grid={sg}x{segs} block=64")
            rec = segs * SLOTS * N * 8
        else:
            parts.append(f"ind_scan_seq_kernel walks={walks} grid={sg} block=64")
    if stoch:
        parts.append(f"ind_fastk_kernel grid={fg} block={BLOCK}")
    if n_window:
        parts.append(f"ind_window_kernel ops={n_window} grid={wg} block={BLOCK}")
    return " | ".join(parts), rec + (T * N * 8 if stoch else 0)


DEFAULT = [(n, {}) for n in ("ema", "bbands", "macd", "atr", "rsi", "adx", "dx", "stoch", "cci", "obv", "adosc")]
SPECS = [DEFAULT, [("ema", {}), ("ema", {"timeperiod": 60}), ("ema", {"timeperiod": 90}), ("rsi", {})],
         [("bbands", {}), ("cci", {})], [("obv", {})], [("stoch", {})], [("adx", {"timeperiod": 256}), ("macd", {})]]
TS = (1, 2, 33, 34, 35, 34 + 63, 34 + 64, 34 + 65, 400, 5000, 5033, 33 + 64 * 32, 33 + 64 * 32 + 1, 33 + 64 * 33, 1 << 20)
NS = (1, 63, 64, 65, 510, SPLIT_MAX_COLS - 1, SPLIT_MAX_COLS, SPLIT_MAX_COLS + 1, 65536 * 30, 0, -3)


@functools.lru_cache(maxsize=None)
def plan_cases():
    cases = [(T, N, i) for i in range(len(SPECS)) for T, N in itertools.product(TS, NS)]
    cases += [(I32_MAX, I32_MAX, 0), (I32_MAX, 1, 0), (600, I32_MAX, 3), (-1, 4, 0), (511 + 64, 8, 5), (511 + 63, 8, 5)]
    return cases


def test_path_and_workspace_match_the_transcribed_plan():
    lib = _abi.load()
    seen = set()
    for T, N, i in plan_cases():
        ops, _ = features.indicator_ops(SPECS[i])
        text, work = expected_path(T, N, SPECS[i])
        assert lib.pmenv_ind_path(T, N, ops, len(ops)).decode() == text, (T, N, i)
        assert lib.pmenv_ind_workspace(T, N, ops, len(ops)) == work, (T, N, i)
        seen |= {part.split(" ")[0] for part in text.split(" | ")}
    assert seen == {"", "ind_scan_seq_kernel", "ind_scan_split_kernel", "ind_fastk_kernel", "ind_window_kernel"}
    got = features.indicator_path(5000, 510, DEFAULT)                  # the reference's shape: the split form
    assert got[0] == ("ind_scan_split_kernel", {"walks": 1, "seg": 78, "segs": 64, "grid": (8, 64), "block": 64})
    assert [n for n, _ in got] == ["ind_scan_split_kernel", "ind_fastk_kernel", "ind_window_kernel"]
    assert features.indicator_path(306, 65536 * 30, DEFAULT)[0] == \
        ("ind_scan_seq_kernel", {"walks": 1, "grid": 30720, "block": 64})   # the per-env series: the sequential form
    assert features.indicator_path(10, 4, DEFAULT) == []


def test_apply_refuses_on_the_host_before_any_launch():
    """every PMENV_ERR_ARG case is decided from the arguments' values (host buffers here:
    nothing is launched)"""
    lib = _abi.load()
    buf = (ctypes.c_float * 65536)()
    base = ctypes.addressof(buf)
    p = lambda off: ctypes.c_void_p(base + 4 * off)  # noqa: E731
    ops, _ = features.indicator_ops(DEFAULT)
    K, L, _ = features.indicator_layout(DEFAULT)
    T, N, C = 40, 4, 5
    chan = (ctypes.c_int32 * 5)(0, 1, 2, 3, 4)
    nbytes = lib.pmenv_ind_workspace(T, N, ops, len(ops))
    assert nbytes == T * N * 8                                          # stoch's stream; too short to split
    work = ctypes.c_void_p(base + 4 * 32768)
    out = p(T * N * C)

    def call(bars=p(0), T=T, N=N, C=C, chan=chan, ops=ops, n_ops=len(ops), out=out, ldo=K, col0=0, work=work,
             nbytes=nbytes):
        return lib.pmenv_ind_apply(bars, T, N, C, chan, ops, n_ops, out, ldo, col0, work, nbytes, None)

    assert call(T=L) == -1 and call(T=L - 1) == -1 and call(T=0) == -1
    assert call(N=0) == -1 and call(C=0) == -1
    assert call(chan=(ctypes.c_int32 * 5)(0, 1, 2, 3, -1)) == -1 and call(chan=(ctypes.c_int32 * 5)(0, 5, 2, 3, 4)) == -1
    assert call(ldo=K - 1) == -1 and call(ldo=K + 1, col0=2) == -1 and call(col0=-1, ldo=K + 4) == -1
    assert call(out=p(0)) == -1 and call(out=p(T * N * C - 1)) == -1
    assert call(bars=p((T - L) * N * K - 1), out=p(0)) == -1            # out ends inside bars
    assert call(nbytes=nbytes - 1) == -1 and call(work=None) == -1
    assert call(work=ctypes.c_void_p(base + 4 * 32768 + 4)) == -1       # a misaligned workspace
    assert call(bars=None) == -1 and call(out=None) == -1 and call(chan=None) == -1 and call(ops=None) == -1
    assert call(n_ops=0) == -1 and call(n_ops=33) == -1
    assert call(bars=ctypes.c_void_p(base + 2)) == -4 and call(out=ctypes.c_void_p(base + 4 * T * N * C + 1)) == -4


# ---------------------------------------------------------------- the header on its own
def compile_sweep(tmp_path, name, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, SWEEP_SRC], check=True)
    return out


def _raw_ops():
    """(kind, p, f) lists for the layout lines: every kind at its edges, and bad ones"""
    cases = [[(k, (14, 14, 14), (2.0, 2.0))] for k in range(-1, 13)]
    cases += [[(k, (b, 14, 14), (2.0, 2.0))] for k in range(11) for b in (1, 2, 256, 257, -I32_MAX - 1, I32_MAX)]
    cases += [[(2, (26, 12, b), (0.0, 0.0))] for b in (1, 2, 256, 257)]
    cases += [[(7, (5, b, 3), (0.0, 0.0))] for b in (1, 2, 256, 257)]
    cases += [[(0, (30, 0, 0), (0.0, 0.0))] * n for n in (0, 1, 32, 33)]
    cases += [[(0, (30, 0, 0), (0.0, 0.0)), (11, (30, 0, 0), (0.0, 0.0))]]
    return cases


def _line(kind, T, N, ops):
    return f"{kind} {T} {N} {len(ops)} " + " ".join(f"{k} {p[0]} {p[1]} {p[2]} {f[0]!r} {f[1]!r}" for k, p, f in ops) + "\n"


def _arr(ops):
    arr = (_abi.PmenvIndOp * max(len(ops), 1))()
    for a, (k, p, f) in zip(arr, ops):
        a.kind = k
        a.p[:] = p
        a.f[:] = f
    return arr


def _spec_ops(spec):
    ops, _ = features.indicator_ops(spec)
    return [(o.kind, tuple(o.p), tuple(o.f)) for o in ops]


def sweep_input_and_library_lines():
    lib = _abi.load()
    text, lines = "", []
    for ops in _raw_ops():
        K, L = ctypes.c_int32(-1), ctypes.c_int32(-1)
        rc = lib.pmenv_ind_layout(_arr(ops) if ops else None, len(ops), ctypes.byref(K), ctypes.byref(L))
        text += _line("L", 0, 0, ops)
        lines.append(f"{rc} {K.value} {L.value}")
    for T, N, i in plan_cases():
        ops = _spec_ops(SPECS[i])
        arr = _arr(ops)
        text += _line("P", T, N, ops) + _line("W", T, N, ops)
        lines += [lib.pmenv_ind_path(T, N, arr, len(ops)).decode(), str(lib.pmenv_ind_workspace(T, N, arr, len(ops)))]
    return text, lines


def run_sweep(binary, text):
    r = subprocess.run([binary], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[-1] == ""
    return lines[:-1]


def test_header_compiles_without_hip_and_agrees_with_the_library(tmp_path):
    text, lines = sweep_input_and_library_lines()
    assert run_sweep(compile_sweep(tmp_path, "ind_plan_sweep"), text) == lines


def test_header_is_clean_under_the_sanitizers(tmp_path):
    """the same program under -fsanitize=address,undefined (the runtimes linked into it), as its
    own process: no report — the op array holds exactly n_ops ops — and the same lines"""
    binary = compile_sweep(tmp_path, "ind_plan_sweep_san", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan")
    text, lines = sweep_input_and_library_lines()
    assert run_sweep(binary, text) == lines
