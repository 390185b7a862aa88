"""The ADF reference (tests/adf_ref.py) and the ADF plan (csrc/adf_plan.h) on the CPU: the
reference against the closed form of simple regression, its invariance under x -> a x + b,
MacKinnon's p-value at its textbook points, the integer lag rule against the float formula,
the search's termination cases, the conditions the GPU test's inputs must meet (they are
conditions on the inputs, checked on the reference alone), and adf_plan.h through
tests/host/adf_plan_sweep.cpp, compiled with the plain host C++ compiler — and once more
under the address and undefined-behaviour sanitizers, run as its own process — which must
print what the library returns. Nothing here touches a device."""
import functools
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import adf_ref
from pmenv import _abi, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_SRC = os.path.join(ROOT, "tests", "host", "adf_plan_sweep.cpp")
I32_MAX = 2 ** 31 - 1
TILE, CHUNK, MAX_LAG = 8, 256, 64


# ---------------------------------------------------------------- the reference itself
def test_lag_zero_equals_the_closed_form_of_simple_regression():
    rng = np.random.default_rng(1)
    for n in (16, 50, 333):
        x = np.cumsum(rng.standard_normal(n)).astype(np.float32)
        r = adf_ref.adf(x, maxlag=0)
        x64 = x.astype(np.float64)
        lvl, dif = x64[:-1], np.diff(x64)
        sxx = np.sum((lvl - lvl.mean()) ** 2)
        beta = np.sum((lvl - lvl.mean()) * (dif - dif.mean())) / sxx
        res = dif - dif.mean() - beta * (lvl - lvl.mean())
        want = beta / math.sqrt(res @ res / (n - 1 - 2) / sxx)
        assert r["status"] == adf_ref.OK and r["usedlag"] == 0 and r["nobs"] == n - 1
        assert abs(r["stat"] - want) <= 1e-12 * max(1.0, abs(want)), (n, r["stat"], want)


def test_stat_and_usedlag_are_invariant_under_positive_affine_maps():
    y, first, _ = adf_ref.catalogue(300)
    for c in range(12):
        x = np.round(y[first[c]:, c].astype(np.float64) * 1024.0) / 1024.0   # |x| < 2^8 on a 2^-10 grid: the maps
        assert np.abs(x).max() < 256.0                                       # below are exact in f32
        base = adf_ref.adf(x)
        for a, b in ((2.0, 0.0), (0.5, 3.0), (4.0, -16.0)):
            r = adf_ref.adf(a * x + b)
            assert r["usedlag"] == base["usedlag"] and r["nobs"] == base["nobs"]
            assert abs(r["stat"] - base["stat"]) <= 1e-9 * max(1.0, abs(base["stat"])), (c, a, b)


def test_pvalue_sanity_points():
    for s, p in ((-3.43, 0.01), (-2.86, 0.05), (-2.57, 0.10)):
        assert abs(adf_ref.pvalue(s) - p) <= 1e-3, (s, adf_ref.pvalue(s))
    below = adf_ref.pvalue(-1.61)
    above = adf_ref.pvalue(math.nextafter(-1.61, 0.0))
    assert abs(below - above) <= 1e-3
    assert adf_ref.pvalue(2.75) == 1.0 and adf_ref.pvalue(-18.84) == 0.0 and math.isnan(adf_ref.pvalue(math.nan))
    lib = _abi.load()
    for s in (-20.0, -18.83, -5.0, -3.43, -2.86, -1.61, -1.6, 0.0, 2.74, 2.75, 3.0):
        assert abs(lib.pmenv_adf_pvalue(s) - adf_ref.pvalue(s)) <= 1e-15, s
    assert math.isnan(lib.pmenv_adf_pvalue(math.nan))


def test_integer_lag_rule_equals_the_float_formula():
    """over n = 4 .. 100,000, except that the integer rule is exact where the float one may not
    be: at n = 100 m^4 / 20736 exactly (100, 1,600, 8,100 ...) the ceiling is m itself"""
    lib = _abi.load()
    n = np.arange(4, 100001, dtype=np.int64)
    flt = np.minimum(n // 2 - 2, np.ceil(12.0 * (n / 100.0) ** 0.25).astype(np.int64))
    exact = {100 * m ** 4 // 20736: m for m in range(1, 80) if (100 * m ** 4) % 20736 == 0}
    assert {100, 1600, 8100} <= set(exact)
    got = np.array([lib.pmenv_adf_maxlag(int(v), -1) for v in n])
    for v, m in exact.items():
        if 4 <= v <= 100000:
            assert got[v - 4] == min(v // 2 - 2, m), v
            flt[v - 4] = got[v - 4]
    assert np.array_equal(got, flt)
    assert all(adf_ref.maxlag_rule(int(v)) == g for v, g in zip(n[:5000], got[:5000]))
    for v, ml, want in ((400, 0, 0), (400, 7, 7), (400, 500, 198), (16, 64, 6), (3, 5, 0), (400, -1, 17)):
        assert lib.pmenv_adf_maxlag(v, ml) == want == adf_ref.maxlag_of(v, None if ml < 0 else ml), (v, ml)


def test_numpy_weights_equal_the_library_bit_for_bit():
    for T, thres in ((300, 1e-5), (400, 1e-2), (6000, 1e-5)):
        for d in (0.0, 2.0 ** -17, 1e-5, 0.05, 0.3, 0.5, 0.75, 1 - 2.0 ** -16, 1.0):
            taps, w = features.ffd_weights(d, thres, T)
            ref, wr = adf_ref.numpy_weights(d, thres, T)
            assert w == wr and np.array_equal(taps.view(np.uint32), ref.view(np.uint32)), (T, thres, d)


# ---------------------------------------------------------------- the search's termination
def _const_test(p, status=adf_ref.OK):
    return lambda x: dict(status=status, pvalue=p, stat=0.0)


def test_search_termination_cases():
    x = adf_ref.search_input()[:, 0]
    d, info = adf_ref.search(x, 1e-2, adf_ref.numpy_weights, _const_test(0.0))       # always stationary
    assert d == 0.0 and info["evals"] == 16
    d, info = adf_ref.search(x, 1e-2, adf_ref.numpy_weights, _const_test(1.0))       # never stationary
    assert d == 1.0 - 2.0 ** -16 and info["evals"] == 16
    d, info = adf_ref.search(x, 1e-2, adf_ref.numpy_weights, _const_test(0.0495))    # inside the band at once
    assert d == 0.5 and info["evals"] == 1
    hits = iter((1.0, 0.0, 0.05))                                                     # 0.5 up, 0.75 down, 0.625 in the band
    d, info = adf_ref.search(x, 1e-2, adf_ref.numpy_weights, lambda s: dict(status=0, pvalue=next(hits), stat=0.0))
    assert d == 0.625 and info["evals"] == 3
    d, info = adf_ref.search(x, 1e-2, adf_ref.numpy_weights, _const_test(math.nan, adf_ref.DEGENERATE))
    assert d == 0.5 and info["evals"] == 1                                            # a NaN p ends the column
    d, info = adf_ref.search(x, 1e-2, adf_ref.numpy_weights, _const_test(math.nan, adf_ref.TOO_SHORT))
    assert d == 1.0 - 2.0 ** -16 and info["evals"] == 16                              # TOO_SHORT counts as p = 1
    assert adf_ref.search(x, 1e-2, adf_ref.numpy_weights, d_init=0.4)[0] == 0.4
    assert adf_ref.search(x, 1e-2, adf_ref.numpy_weights, active=False)[0] == 0.0


# ---------------------------------------------------------------- conditions on the GPU test's inputs
@pytest.mark.parametrize("T", adf_ref.TS)
def test_catalogue_meets_the_input_conditions(T):
    """every catalogue case (the leading C columns of the T-row table): the best and the
    second-best AIC at least 1e-6 apart, tol below 1e-7, every column testable, an AR(2) column
    whose best lag is at least 1, per-column firsts among the FFD columns"""
    y, first, kinds = adf_ref.catalogue(T)
    ref = adf_ref.catalogue_ref(T)
    assert np.all(ref["status"] == adf_ref.OK)
    assert ref["aic_gap"].min() >= 1e-6
    assert ref["tol"].max() < 1e-7 and np.all(ref["tol"] > 0)
    ar2 = [c for c, k in enumerate(kinds) if k == "ar2"]
    assert np.all(ref["usedlag"][ar2] >= 1)
    assert len({int(first[c]) for c, k in enumerate(kinds) if k == "ffd"}) == 3
    assert np.all(np.isnan(y[0, first > 0])) and np.all(np.isfinite(y[-1]))
    for C in adf_ref.CS:
        assert set(kinds[:C]) == set(adf_ref.KINDS[:min(C, 6)])


def test_the_reference_agrees_with_a_longdouble_solve_well_inside_tol():
    """the reference's own error: lstsq on the uncentred design against Gauss-Jordan on the
    centred normal equations in np.longdouble, over the catalogue and the given-lag cases of
    the GPU test — a tenth of tol at the most, so the kernel's bound measures the kernel"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here")
    for T in adf_ref.TS:
        y, first, _ = adf_ref.catalogue(T)
        ref = adf_ref.catalogue_ref(T)
        for c in range(y.shape[1]):
            want = adf_ref.stat_longdouble(y[first[c]:, c], int(ref["usedlag"][c]))
            assert abs(ref["stat"][c] - want) <= 0.1 * ref["tol"][c], (T, c)
    y, first, _ = adf_ref.catalogue(300)
    for autolag, maxlag in ((False, None), (False, 0), (False, 1), (False, 7), (True, 1), (True, 7)):
        for c in range(12):
            r = adf_ref.adf(y[first[c]:, c], maxlag, autolag)
            assert abs(r["stat"] - adf_ref.stat_longdouble(y[first[c]:, c], r["usedlag"])) <= 0.1 * r["tol"], (maxlag, c)


@pytest.mark.parametrize("thres", adf_ref.SEARCH_THRESES)
def test_search_inputs_stay_clear_of_the_band_edges(thres):
    d, infos = adf_ref.search_ref(thres)
    ps = np.array([p for i in infos for p in i["ps"]])
    assert ps.size and np.abs(ps - adf_ref.P_HIGH).min() >= 1e-6 and np.abs(ps - adf_ref.P_LOW).min() >= 1e-6
    assert all(i["evals"] <= 16 for i in infos)
    if thres == adf_ref.SEARCH_THRESES[0]:
        assert any(0 < i["evals"] < 16 for i in infos) and np.any(d == 0.0) and np.any(d > 0.0)
    else:                                       # wide filters on a short series: probes too short to test
        assert any(p == 1.0 for i in infos for p in i["ps"])


# ---------------------------------------------------------------- the plan
def plan(R, C, maxlag):
    if R < 1 or C < 1 or maxlag > MAX_LAG:
        return None
    kcap = adf_ref.maxlag_of(R, None if maxlag < 0 else maxlag)
    if kcap > MAX_LAG:
        return None
    doubles = (kcap + 1) * (kcap + 2) // 2 + (kcap + 2) * (kcap + 3) // 2 + 7 * (kcap + 2)
    return dict(kcap=kcap, work=C * (2 * kcap + 7) * 8, sums_grid=-(-C // TILE), lds=doubles * 8)


def expected(R, C, maxlag):
    p = plan(R, C, maxlag)
    if p is None:
        return "", 0
    return (f"adf_sums_kernel tile={TILE} chunk={CHUNK} kcap={p['kcap']} grid={p['sums_grid']} block={64 * TILE} | "
            f"adf_solve_kernel kcap={p['kcap']} lds={p['lds']} grid={C} block=64"), p["work"]


RS = (0, 1, 3, 15, 16, 17, 100, 101, 300, 400, 1600, 5000, 80908, 80909, 100000, I32_MAX)
CS = (0, 1, 5, 7, 8, 9, 64, 65, 130, 2000, I32_MAX)
MLS = (-1, 0, 1, 7, 64, 65, 1000)


@functools.lru_cache(maxsize=None)
def plan_cases():
    return [c for c in itertools.product(RS, CS, MLS)] + [(-1, 4, -1), (4, -1, -1), (400, 4, -5)]


def test_adf_path_and_workspace_match_the_transcribed_plan():
    lib = _abi.load()
    seen = set()
    for R, C, ml in plan_cases():
        text, work = expected(R, C, ml)
        assert lib.pmenv_adf_path(R, C, ml).decode() == text, (R, C, ml)
        assert lib.pmenv_adf_workspace(R, C, ml) == work, (R, C, ml)
        seen.add(bool(text))
    assert seen == {True, False}
    assert lib.pmenv_adf_path(80908, 4, -1) and not lib.pmenv_adf_path(80909, 4, -1)   # the rule passes 64 there
    assert features.adf_path(400, 130) == [
        ("adf_sums_kernel", {"tile": 8, "chunk": 256, "kcap": 17, "grid": 17, "block": 512}),
        ("adf_solve_kernel", {"kcap": 17, "lds": plan(400, 130, -1)["lds"], "grid": 130, "block": 64})]
    assert features.adf_path(0, 4) == []


def compile_sweep(tmp_path, name, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, SWEEP_SRC], check=True)
    return out


LAG_CASES = [(n, ml) for n in (0, 3, 4, 15, 16, 17, 99, 100, 101, 1599, 1600, 1601, 8100, 8101, 80908, 80909, I32_MAX)
             for ml in (-1, 0, 7, 64, 1000)]
STATS = (-25.0, -18.83, -18.829, -6.5, -3.43, -2.86, -2.57, -1.61, -1.6099, -0.3, 0.0, 1.2, 2.74, 2.7401, 9.0)


def library_lines():
    lib = _abi.load()
    out = [str(lib.pmenv_adf_maxlag(n, ml)) for n, ml in LAG_CASES]
    out += [np.float64(lib.pmenv_adf_pvalue(s)).view(np.uint64).item().to_bytes(8, "big").hex() for s in STATS]
    out += [f"{lib.pmenv_adf_path(R, C, ml).decode()}|{lib.pmenv_adf_workspace(R, C, ml)}" for R, C, ml in plan_cases()]
    return out


def run_sweep(binary):
    text = "".join(f"M {n} {ml}\n" for n, ml in LAG_CASES)
    text += "".join(f"V {s!r}\n" for s in STATS)
    text += "".join(f"P {R} {C} {ml}\n" for R, C, ml in plan_cases())
    r = subprocess.run([binary], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[-1] == ""
    return lines[:-1]


def test_header_compiles_without_hip_and_agrees_with_the_library(tmp_path):
    """The plain host compiler builds a program from adf_plan.h alone (no HIP include path, no
    library), and it prints the library's lag bounds, p-values, paths and workspace sizes."""
    assert run_sweep(compile_sweep(tmp_path, "adf_plan_sweep")) == library_lines()


def test_header_is_clean_under_the_sanitizers(tmp_path):
    """The same program under -fsanitize=address,undefined (the runtimes linked into it), as its
    own process: no report, and the same lines."""
    binary = compile_sweep(tmp_path, "adf_plan_sweep_san", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan")
    assert run_sweep(binary) == library_lines()
