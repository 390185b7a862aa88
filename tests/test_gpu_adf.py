"""The search for the orders of differencing on the GPU (pmenv.features.adf / find_d;
csrc/adf.h): pmenv_adf against the numpy restatement of its definitions (tests/adf_ref.py:
lstsq on the uncentred design, another formulation than the kernel's centred normal
equations) over the catalogue test_adf_host.py has checked the input conditions of —
usedlag, nobs and status equal, stat within
    tol = 4 (nobs + 8 p) kappa_2 2^-53 max(1, |stat|),
the forward bound of a Cholesky solve plus the Gram sums with kappa_2 the condition number
numpy computes for the centred, column-normalised design of the final fit (from the reference
per column, not fitted to the kernel), pvalue within 2 tol + 1e-15 — its independence of the
other columns, of first and of the workspace's contents, its statuses and refusals,
pmenv_ffd_table against pmenv_ffd_weights bit for bit, find_d against the reference search,
one captured round replayed on fresh data, and build(d="auto"). Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import adf_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT_F, SENT_I = 12345.0, 1234567
NAMES = ("stat", "pvalue", "usedlag", "nobs", "status")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _expected_path(R, C, maxlag=None):
    kcap = adf_ref.maxlag_of(R, maxlag)
    doubles = (kcap + 1) * (kcap + 2) // 2 + (kcap + 2) * (kcap + 3) // 2 + 7 * (kcap + 2)
    return [("adf_sums_kernel", {"tile": 8, "chunk": 256, "kcap": kcap, "grid": -(-C // 8), "block": 512}),
            ("adf_solve_kernel", {"kcap": kcap, "lds": 8 * doubles, "grid": C, "block": 64})]


def _adf_raw(y, first=None, maxlag=-1, autolag=1, ld=None, fill="nan"):
    """pmenv_adf through the raw ABI: y [R, C] placed in rows of ld floats between two guard
    rows, every output between two sentinels, the workspace filled as `fill` says. Returns the
    five outputs as numpy arrays after checking that nothing around them was written."""
    from pmenv import _abi, features
    lib = _abi.load()
    R, C = y.shape
    ld = C if ld is None else ld
    assert features.adf_path(R, C, None if maxlag < 0 else maxlag) == \
        _expected_path(R, C, None if maxlag < 0 else maxlag)      # names and geometry before any value
    buf = torch.full((R + 2, ld), SENT_F, dtype=torch.float32, device=DEV)
    buf[1:R + 1, :C] = torch.from_numpy(np.ascontiguousarray(y))
    before = buf.clone()
    outs = {k: torch.full((C + 2,), SENT_F if k in ("stat", "pvalue") else SENT_I,
                          dtype=torch.float64 if k in ("stat", "pvalue") else torch.int32, device=DEV) for k in NAMES}
    nbytes = lib.pmenv_adf_workspace(R, C, maxlag)
    assert nbytes == C * (2 * adf_ref.maxlag_of(R, None if maxlag < 0 else maxlag) + 7) * 8
    work = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=DEV)
    if fill == "nan":
        work.fill_(float("nan"))
    elif fill == "zero":
        work.zero_()
    else:
        work.copy_(torch.from_numpy(np.random.default_rng(5).standard_normal(work.numel()) * 1e30))
    work[0], work[-1] = SENT_F, SENT_F
    fst = None if first is None else torch.from_numpy(np.ascontiguousarray(first, dtype=np.int32)).to(DEV)
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n * t.element_size())  # noqa: E731
    rc = lib.pmenv_adf(off(buf, ld), R, C, ld, _p(fst) if fst is not None else None, maxlag, autolag,
                       off(outs["stat"], 1), off(outs["pvalue"], 1), off(outs["usedlag"], 1), off(outs["nobs"], 1),
                       off(outs["status"], 1), off(work, 1), nbytes,
                       ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))            # y and its guard rows
    assert work[0].item() == SENT_F and work[-1].item() == SENT_F
    res = {}
    for k, t in outs.items():
        a = t.cpu().numpy()
        assert a[0] == a[-1] == (SENT_F if k in ("stat", "pvalue") else SENT_I), k
        res[k] = a[1:-1].copy()
    return res


def _check(got, ref, cols=slice(None)):
    """the discrete outputs equal, stat and pvalue within the reference's own bound"""
    for k in ("usedlag", "nobs", "status"):
        assert np.array_equal(got[k], ref[k][cols]), k
    ok = ref["status"][cols] == adf_ref.OK
    tol = ref["tol"][cols][ok]
    assert np.all(np.abs(got["stat"][ok] - ref["stat"][cols][ok]) <= tol), \
        (np.abs(got["stat"][ok] - ref["stat"][cols][ok]) / tol).max()
    assert np.all(np.abs(got["pvalue"][ok] - ref["pvalue"][cols][ok]) <= 2 * tol + 1e-15)
    assert np.all(np.isnan(got["stat"][~ok])) and np.all(np.isnan(got["pvalue"][~ok]))


def _same_bits(a, b):
    for k in NAMES:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


# ---------------------------------------------------------------- the statistic
@pytest.mark.parametrize("C", adf_ref.CS)
@pytest.mark.parametrize("T", adf_ref.TS)
def test_adf_equals_the_reference_over_the_catalogue(T, C):
    y, first, _ = adf_ref.catalogue(T)
    ref = adf_ref.catalogue_ref(T)
    got = _adf_raw(y[:, :C], first[:C], ld=C + (3 if C % 2 else 0))
    _check(got, ref, slice(0, C))
    assert np.all(got["status"] == adf_ref.OK)


def test_a_column_alone_among_130_and_at_another_first_has_the_same_bits():
    y, first, _ = adf_ref.catalogue(400)
    whole = _adf_raw(y, first)
    for c in (0, 3, 4, 5, 11, 17, 64, 65, 129):
        pick = {k: whole[k][c:c + 1] for k in NAMES}
        _same_bits(_adf_raw(y[:, c:c + 1], first[c:c + 1]), pick)
        col = y[first[c]:, c:c + 1]
        _same_bits(_adf_raw(col), pick)                                   # first = 0, NULL
        pad = np.concatenate([np.full((300, 1), np.nan, dtype=np.float32), col])
        _same_bits(_adf_raw(pad, np.array([300])), pick)                  # rows past one staging chunk in front


@pytest.mark.parametrize("autolag,maxlag", [(0, -1), (0, 0), (0, 1), (0, 7), (1, 0), (1, 1), (1, 7)])
def test_given_lag_bounds_and_autolag_off(autolag, maxlag):
    y, first, _ = adf_ref.catalogue(300)
    y, first = y[:, :12], first[:12]
    ref = adf_ref.adf_columns(y, first, None if maxlag < 0 else maxlag, bool(autolag))
    assert np.all(ref["tol"] < 1e-7) and (autolag == 0 or maxlag == 0 or ref["aic_gap"].min() >= 1e-6)
    got = _adf_raw(y, first, maxlag, autolag)
    _check(got, ref)
    if not autolag:
        want = adf_ref.maxlag_of(300, None if maxlag < 0 else maxlag)
        assert np.all(got["usedlag"][first == 0] == want)


def test_lengths_either_side_of_16_rows_and_of_a_lag_step():
    y, _, _ = adf_ref.catalogue(400)
    y = np.ascontiguousarray(y[-101:, :4])                                # walk, drift, two AR(1): no NaN rows left
    assert np.all(np.isfinite(y))
    first = np.array([1, 0, 86, 85], dtype=np.int32)                      # n = 100, 101, 15, 16
    ref = adf_ref.adf_columns(y, first)
    assert [adf_ref.maxlag_rule(n) for n in (100, 101, 15, 16)] == [12, 13, 5, 6]
    assert ref["status"].tolist() == [0, 0, adf_ref.TOO_SHORT, 0]
    assert ref["aic_gap"].min() >= 1e-6 and np.nanmax(ref["tol"]) < 1e-7
    got = _adf_raw(y, first)
    _check(got, ref)
    assert got["nobs"][2] == 0 and got["usedlag"][2] == 0
    beyond = _adf_raw(y, np.array([101, 500, -3, 100], dtype=np.int32))   # clamped to [0, R]: n = 0, 0, 101, 1
    assert beyond["status"].tolist() == [1, 1, 0, 1]
    _same_bits({k: beyond[k][2:3] for k in NAMES}, _adf_raw(y[:, 2:3]))


def test_degenerate_columns_and_a_nan_are_confined_to_their_column():
    y, first, _ = adf_ref.catalogue(300)
    y, first = y[:, :10].copy(), first[:10].copy()
    clean = _adf_raw(y, first)
    bad = y.copy()
    bad[:, 1] = 2.5                                                       # a constant column
    bad[:, 3] = 3.0 + 0.5 * np.arange(300, dtype=np.float32)              # a pure ramp, exact in f32
    bad[150, 6] = np.nan                                                  # one NaN
    bad[299, 8] = np.inf                                                  # an inf in the last row
    first[1] = first[3] = 0
    ref = adf_ref.adf_columns(bad, first)
    assert ref["status"].tolist() == [0, 2, 0, 2, 0, 0, 2, 0, 2, 0]
    got = _adf_raw(bad, first)
    _check(got, ref)
    keep = [0, 2, 4, 5, 7, 9]
    _same_bits({k: got[k][keep] for k in NAMES}, {k: clean[k][keep] for k in NAMES})
    head = y.copy()
    head[first[0], 0] = np.nan                                            # the column's first row
    head[first[2] + 5, 2] = -np.inf                                       # a row only the lagged differences read
    got = _adf_raw(head, first)
    assert got["status"].tolist()[:3] == [2, clean["status"][1], 2]
    _same_bits({k: got[k][3:] for k in NAMES}, {k: clean[k][3:] for k in NAMES})


def test_the_workspace_contents_do_not_matter():
    y, first, _ = adf_ref.catalogue(300)
    base = _adf_raw(y[:, :65], first[:65], fill="nan")
    for fill in ("zero", "garbage"):
        _same_bits(_adf_raw(y[:, :65], first[:65], fill=fill), base)


def test_refusals_return_their_codes():
    from pmenv import _abi
    lib = _abi.load()
    R, C = 64, 4
    y = torch.zeros(R * C + 8, dtype=torch.float32, device=DEV)
    f64 = torch.zeros(2 * C + 2, dtype=torch.float64, device=DEV)
    i32 = torch.zeros(3 * C + 2, dtype=torch.int32, device=DEV)
    nbytes = lib.pmenv_adf_workspace(R, C, -1)
    work = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=DEV)
    at = lambda t, n, b=0: ctypes.c_void_p(t.data_ptr() + n * t.element_size() + b)  # noqa: E731

    def call(**kw):
        a = dict(y=at(y, 0), R=R, C=C, ld=C, first=None, maxlag=-1, autolag=1, stat=at(f64, 0), pvalue=at(f64, C),
                 usedlag=at(i32, 0), nobs=at(i32, C), status=at(i32, 2 * C), work=at(work, 0), nbytes=nbytes)
        a.update(kw)
        return lib.pmenv_adf(a["y"], a["R"], a["C"], a["ld"], a["first"], a["maxlag"], a["autolag"], a["stat"],
                             a["pvalue"], a["usedlag"], a["nobs"], a["status"], a["work"], a["nbytes"], None)

    assert call() == 0
    for kw in (dict(y=None), dict(stat=None), dict(pvalue=None), dict(usedlag=None), dict(nobs=None),
               dict(status=None), dict(work=None), dict(R=0), dict(C=0), dict(ld=C - 1), dict(maxlag=65),
               dict(nbytes=nbytes - 8), dict(work=at(work, 0, 4)), dict(R=80909)):
        assert call(**kw) == -1, kw
    for kw in (dict(y=at(y, 0, 2)), dict(stat=at(f64, 0, 4)), dict(pvalue=at(f64, C, 4)), dict(usedlag=at(i32, 0, 2)),
               dict(first=at(i32, 0, 1))):
        assert call(**kw) == -4, kw
    torch.cuda.synchronize()
    d = torch.zeros(4, dtype=torch.float64, device=DEV)
    taps = torch.zeros(40, dtype=torch.float32, device=DEV)
    wid = torch.zeros(4, dtype=torch.int32, device=DEV)

    def tab(**kw):
        a = dict(d=_p(d), thres=1e-5, T=11, C=4, cap=10, taps=_p(taps), width=_p(wid))
        a.update(kw)
        return lib.pmenv_ffd_table(a["d"], a["thres"], a["T"], a["C"], a["cap"], a["taps"], a["width"], None)

    assert tab() == 0
    for kw in (dict(d=None), dict(width=None), dict(taps=None), dict(T=1), dict(C=0), dict(cap=-1),
               dict(thres=-1.0), dict(thres=float("nan"))):
        assert tab(**kw) == -1, kw
    assert tab(d=at(d, 0, 4)) == -4 and tab(taps=at(taps, 0, 2)) == -4
    st = [torch.zeros(4, dtype=torch.float64, device=DEV) for _ in range(4)]
    it = [torch.zeros(4, dtype=torch.int32, device=DEV) for _ in range(3)]
    upd = lambda p, s, a, th=1e-5, C=4, low=_p(st[0]): lib.pmenv_adf_search_update(  # noqa: E731
        p, s, a, th, C, low, _p(st[1]), _p(st[2]), _p(it[0]), _p(it[1]), _p(it[2]), None, _p(st[3]), None)
    assert upd(None, None, None) == 0
    assert upd(_p(d), None, None) == -1 and upd(None, None, None, 0.0) == -1 and upd(None, None, None, 1e-5, 0) == -1
    assert upd(None, None, None, low=None) == -1 and upd(None, None, None, low=at(st[0], 0, 4)) == -4
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the tap table
@pytest.mark.parametrize("T", (300, 6000))
def test_ffd_table_equals_ffd_weights_bit_for_bit(T):
    from pmenv import features
    ds = [0.0, 2.0 ** -17, 1e-5] + [0.05 * i for i in range(1, 19)] + [1 - 2.0 ** -16, 1.0]
    ds = ds + ds[:6]                                                      # 29 columns: not a multiple of anything
    cap = T - 1
    guard = torch.full((cap + 2, len(ds)), SENT_F, dtype=torch.float32, device=DEV)
    wid = torch.full((len(ds) + 2,), SENT_I, dtype=torch.int32, device=DEV)
    d = torch.tensor(ds, dtype=torch.float64, device=DEV)
    features.ffd_table(d, 1e-5, T, cap, guard[1:cap + 1], wid[1:-1])
    torch.cuda.synchronize()
    g, w = guard.cpu().numpy(), wid.cpu().numpy()
    assert np.all(g[0] == SENT_F) and np.all(g[-1] == SENT_F) and w[0] == w[-1] == SENT_I
    for c, dv in enumerate(ds):
        taps, width = features.ffd_weights(dv, 1e-5, T)
        assert w[1 + c] == width, (dv, w[1 + c], width)
        assert np.array_equal(g[1:1 + width, c].view(np.uint32), taps.view(np.uint32)), dv
        assert not g[1 + width:cap + 1, c].any(), dv                     # the zeroed tail
    small = torch.full((12, len(ds)), SENT_F, dtype=torch.float32, device=DEV)
    features.ffd_table(d, 1e-5, T, 10, small[1:11], wid[1:-1])            # cap below the widths: cap taps, the full width
    torch.cuda.synchronize()
    s = small.cpu().numpy()
    assert np.all(s[0] == SENT_F) and np.all(s[-1] == SENT_F) and np.array_equal(wid.cpu().numpy(), w)
    taps, width = features.ffd_weights(0.5, 1e-5, T)
    assert width > 10 and np.array_equal(s[1:11, ds.index(0.05 * 10)].view(np.uint32), taps[:10].view(np.uint32))


# ---------------------------------------------------------------- the search
@pytest.mark.parametrize("thres", adf_ref.SEARCH_THRESES)
def test_find_d_equals_the_reference_search(thres):
    from pmenv import features
    x = adf_ref.search_input()
    want, infos = adf_ref.search_ref(thres)
    d, info = features.find_d(torch.from_numpy(x).to(DEV), thres)
    assert d.dtype == np.float64 and np.array_equal(d.view(np.uint64), want.view(np.uint64)), (d, want)
    assert np.array_equal(info["evals"], [i["evals"] for i in infos])
    assert np.array_equal(info["status"], [i["status"] for i in infos])
    assert np.array_equal(info["width"], [adf_ref.numpy_weights(v, thres, x.shape[0])[1] for v in want])
    ref_p = np.array([i["pvalue"] for i in infos])
    ok = ~np.isnan(ref_p)
    assert np.array_equal(np.isnan(info["pvalue"]), ~ok) and np.all(np.abs(info["pvalue"][ok] - ref_p[ok]) <= 1e-7)


def test_find_d_keeps_given_orders_and_masked_columns():
    from pmenv import features
    x = adf_ref.search_input()
    want, _ = adf_ref.search_ref(1e-2)
    d_init = np.zeros(12)
    d_init[[0, 5]] = (0.4, 0.125)
    mask = np.ones(12, dtype=bool)
    mask[[1, 5, 9]] = False
    d, info = features.find_d(torch.from_numpy(x.reshape(400, 3, 4)).to(DEV), 1e-2, d_init=d_init.reshape(3, 4),
                              mask=mask.reshape(3, 4))
    exp = np.where(d_init > 0, d_init, np.where(mask, want, 0.0))
    assert d.shape == (3, 4) and np.array_equal(d.reshape(-1), exp)
    assert np.all(info["evals"].reshape(-1)[[0, 1, 5, 9]] == 0) and np.all(np.isnan(info["pvalue"].reshape(-1)[[0, 1, 5, 9]]))


def test_a_captured_round_replays_on_fresh_data():
    from pmenv import features
    xa = torch.from_numpy(adf_ref.search_input()).to(DEV)
    xb = torch.from_numpy(adf_ref.search_input(seed=11)).to(DEV)
    state = ("low", "high", "d_opt", "active", "evals", "status", "last", "d")

    def fresh(x):
        s = features._Search(x, 1e-2)
        s.update(False)
        return s

    eager = fresh(xb)
    eager.round()
    eager.round()
    s = fresh(xa)
    s.round()                                                            # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.round()
    init = fresh(xb)
    s.xpad[s.cap:] = xb
    for k in state:
        getattr(s, k).copy_(getattr(init, k))
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for k in state:
        a, b = getattr(s, k).cpu().numpy(), getattr(eager, k).cpu().numpy()
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    assert eager.evals.max().item() == 3                                # the first probe's and two rounds'


def test_build_auto_equals_build_with_the_found_orders():
    from pmenv import features
    rng = np.random.default_rng(3)
    T, N = 400, 3
    close = 50.0 * np.exp(np.cumsum(0.01 * rng.standard_normal((T, N)), axis=0))
    raw = np.stack([close * 0.99, close * 1.01, close * 0.98, close, 1e4 * (1 + rng.random((T, N)))], axis=2).astype(np.float32)
    tr, te = features.build(raw, "auto", thres=1e-2, device=DEV)
    feats = torch.from_numpy(raw[1:]).to(DEV)
    mask = np.array([True, True, True, True, False])
    d, _ = features.find_d(feats, 1e-2, mask=mask)
    assert d.shape == (N, 5) and np.all(d[:, 4] == 0.0) and np.any(d[:, :4] > 0.0)
    want = np.array([adf_ref.search(raw[1:, n, c], 1e-2, adf_ref.numpy_weights)[0] if c < 4 else 0.0
                     for n in range(N) for c in range(5)]).reshape(N, 5)
    assert np.array_equal(d, want)
    tr2, te2 = features.build(raw, d, thres=1e-2, device=DEV)
    for a, b in ((tr, tr2), (te, te2)):
        assert np.array_equal(a.d, d) and np.array_equal(b.d, d)
        assert torch.equal(a.bars.view(torch.int32), b.bars.view(torch.int32))
        assert torch.equal(a.relatives.view(torch.int32), b.relatives.view(torch.int32))
        assert a.max_width == b.max_width and torch.equal(a.widths, b.widths)
    tr3, _ = features.build(raw, "auto", thres=1e-2, device=DEV, auto_channels=[3])
    assert np.array_equal(tr3.d[:, 3], d[:, 3]) and not tr3.d[:, [0, 1, 2, 4]].any()
