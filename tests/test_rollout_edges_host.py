"""The rollout edge generator's preconditions (tests/rollout_edge_inputs.py), the GAE
selection rule by name and the oracle's answers on the degenerate metric classes — pinned on
the CPU so that test_gpu_rollout_edges.py cannot pass vacuously. Conditions on the inputs: if
one fails for a shape, the inputs change, not the condition."""
import warnings

import numpy as np
import pytest

import rollout_edge_inputs as ri
from oracle import gae as or_gae, trajectory_metrics as or_metrics

ALL_SHAPES = sorted({(T, B, s) for _, _, T, B, s in ri.GAE_CASES} | set(ri.LOOP_CASES) | set(ri.FALLBACK_CASES))
STRUCTURED = [c for c in range(ri.K) if ri.DONE_CLASSES[c][0] not in ("every", "iid")]


def _small(T, B):
    return min(B, 4 * ri.K)          # the classes repeat with period K: a few periods suffice on the CPU


def test_every_done_class_occurs_where_the_batch_is_wide_enough():
    for T, B, shift in ALL_SHAPES:
        if B >= ri.K:
            assert {ri.done_class(b, shift) for b in range(B)} == set(range(ri.K)), (T, B)
        else:
            assert shift != ri.CLASS["none"] or T == 1, f"({T}, {B}): a narrow batch must name its class"
    for T in (64, 65, 127, 300, 513, 2048):
        _, _, d = ri.gae_batch(T, ri.K, seed=T)
        cnt = d.sum(0)
        assert cnt[ri.CLASS["none"]] == 0 and cnt[ri.CLASS["every"]] == T
        assert cnt[ri.CLASS["last"]] == cnt[ri.CLASS["first"]] == cnt[ri.CLASS["mid"]] == 1
        assert d[T - 1, ri.CLASS["last"]] and d[0, ri.CLASS["first"]] and d[T // 2, ri.CLASS["mid"]]
        assert cnt[ri.CLASS["whole_chunk"]] == max(0, min(T, 128) - 64)
        assert np.array_equal(np.unique(d), [0, 1])


def _boundary_hits(d, shift, parts):
    """(a structured env ends an episode on the last day of a piece that has a later piece,
    one on the first day of a piece that has an earlier piece)"""
    last = first = False
    for b in range(d.shape[1]):
        if ri.done_class(b, shift) not in STRUCTURED:
            continue
        for p0, p1 in parts:
            last |= bool(d[p1, b]) and p1 < d.shape[0] - 1
            first |= bool(d[p0, b]) and p0 > 0
    return last, first


@pytest.mark.parametrize("kernel,through,T,B,shift", [c for c in ri.GAE_CASES if c[3] >= ri.K])
def test_dones_sit_on_the_kernels_piece_boundaries(kernel, through, T, B, shift):
    """For the kernel a shape takes: an env (not the every-step class) with an episode end on the
    last day of a segment / chunk / lane chunk and one on the first — and the same for the
    waves' sub-chunks of U days — whenever the horizon has more than one such piece."""
    _, _, d = ri.gae_batch(T, _small(T, B), seed=T * 7 + B, shift=shift)
    if kernel == ri.SCAN:
        parts = ri.scan_pieces(T)
        assert len(parts) == min(64, -(-T // ((T + 63) // 64)))
        assert _boundary_hits(d, shift, parts) == (True, True)
        return
    S, from_end = ri.GEOMETRY[kernel]
    parts = ri.pieces(T, S, from_end)
    if len(parts) > 1:
        assert _boundary_hits(d, shift, parts) == (True, True), (kernel, T)
    U = S // 8
    sub = [(a, min(a + U, p1 + 1) - 1) for p0, p1 in parts for a in range(p0, p1 + 1, U)]
    if len(sub) > 1:
        assert _boundary_hits(d, shift, sub) == (True, True), (kernel, T, "sub-chunks")


def test_narrow_batches_take_a_class_on_their_kernels_boundary():
    """B < K leaves classes out, so the case table names env 0's: it ends an episode on the last or
    the first day of one of its kernel's pieces, inside the horizon."""
    for kernel, _, T, B, shift in ri.GAE_CASES:
        if B >= ri.K:
            continue
        _, _, d = ri.gae_batch(T, B, seed=T * 7 + B, shift=shift)
        parts = ri.scan_pieces(T) if kernel == ri.SCAN else ri.pieces(T, *ri.GEOMETRY[kernel])
        hit = any(d[p1, 0] for _, p1 in parts if p1 < T - 1) or any(d[p0, 0] for p0, _ in parts if p0 > 0)
        assert hit or len(parts) == 1, (kernel, T, B)


def test_scan_kernel_has_empty_lane_chunks_at_257():
    assert len(ri.scan_pieces(257)) == 52          # L = 5: lanes 52 .. 63 own no day


@pytest.mark.parametrize("T,B", [(1, 18), (127, 18), (129, 36), (300, 36), (513, 36), (700, 36), (1100, 36),
                                 (1025, 36)])
@pytest.mark.parametrize("gamma,lam", ri.GAMMA_LAMBDA)
def test_chunked_composition_stays_inside_the_cap(T, B, gamma, lam):
    """A correct chunked composition (numpy f64, every geometry of rollout.h: 64- and 128-day
    pieces from day 0 and from the end) against the oracle's sequential recursion, under the
    criterion the GPU tests apply: the cap is loose for a correct kernel."""
    r, v, d = ri.gae_batch(T, B, seed=T + B)
    oadv, oret = or_gae(r, v, d, gamma, lam)
    for NW, U, from_end in [(8, 8, True), (8, 16, True), (8, 8, False), (8, 16, False)]:
        adv, ret = ri.chunked_gae(r, v, d, gamma, lam, NW, U, from_end)
        ri.compare_gae(adv, oadv, f"adv {NW}x{U} from_end={from_end}")
        ri.compare_gae(ret, oret, f"ret {NW}x{U} from_end={from_end}")


def test_chunked_composition_with_scaled_values():
    r, v, d = ri.gae_batch(700, 36, seed=5)
    v = (v * 25000.0).astype(np.float32)
    oadv, oret = or_gae(r, v, d, 0.99, 0.95)
    for from_end in (True, False):
        adv, ret = ri.chunked_gae(r, v, d, 0.99, 0.95, 8, 8, from_end)
        ri.compare_gae(adv, oadv)
        ri.compare_gae(ret, oret)


def test_the_criterion_rejects_an_f32_intermediate():
    """The same composition with the carry rounded to f32 between chunks fails the criterion:
    the test would notice an f32 intermediate."""
    r, v, d = ri.gae_batch(700, 36, seed=5)
    oadv, _ = or_gae(r, v, d, 0.99, 0.95)
    g, gl = float(np.float32(0.99)), float(np.float32(0.99)) * float(np.float32(0.95))
    n = (d == 0).astype(np.float64)
    v64 = v.astype(np.float64)
    dl = r.astype(np.float64) + g * n * v64[1:] - v64[:-1]
    a = np.zeros(36)
    adv = np.empty((700, 36), np.float32)
    for t in range(699, -1, -1):
        if t % 64 == 63:
            a = a.astype(np.float32).astype(np.float64)
        a = dl[t] + gl * n[t] * a
        adv[t] = a
    with pytest.raises(AssertionError):
        ri.compare_gae(adv, oadv)


@pytest.mark.parametrize("gamma,lam", ri.GAMMA_LAMBDA)
def test_oracle_is_exact_where_the_carry_is_cut(gamma, lam):
    """lambda = 0 (or gamma = 0) everywhere, and the every-step class at any lambda: the oracle
    itself gives f32(delta) bit for bit — the closed form the GPU tests hold the kernels to."""
    r, v, d = ri.gae_batch(300, 2 * ri.K, seed=3)
    oadv, oret = or_gae(r, v, d, gamma, lam)
    eadv, eret = ri.delta_exact(r, v, d, gamma)
    cols = slice(None) if gamma * lam == 0.0 else [b for b in range(2 * ri.K) if b % ri.K == ri.CLASS["every"]]
    assert np.array_equal(oadv[:, cols].view(np.uint32), eadv[:, cols].view(np.uint32))
    assert np.array_equal(oret[:, cols].view(np.uint32), eret[:, cols].view(np.uint32))


def test_done_byte_stamps_and_poison_helpers():
    r, v, d = ri.gae_batch(130, ri.K, seed=1)
    s = ri.stamp_done_bytes(d)
    assert np.array_equal(s != 0, d != 0) and set(np.unique(s)) == {0, 2, 128, 255} and d.max() == 1
    r2, v2 = ri.poison(r, v, "v", 130, 3, "nan")
    assert np.isnan(v2[130, 3]) and np.isfinite(v).all() and np.isnan(v2).sum() == 1 and np.array_equal(r, r2)
    r3, _ = ri.poison(r, v, "r", 0, 0, "-inf")
    assert r3[0, 0] == -np.inf and np.isfinite(r).all()
    # 0 * NaN is NaN: a done does not stop a NaN on its way back through the recursion
    oadv, _ = or_gae(*ri.poison(r, v, "r", 100, ri.CLASS["every"], "nan"), d, 0.99, 0.95)
    assert np.isnan(oadv[:101, ri.CLASS["every"]]).all() and np.isfinite(oadv[101:, ri.CLASS["every"]]).all()
    assert np.isfinite(np.delete(oadv, ri.CLASS["every"], 1)).all()


def test_gae_path_table():
    """pmenv_gae_path against the selection rule as the tests rely on it (host only: needs the
    library, no device)."""
    from pmenv import rollout, _abi
    lib = _abi.load()
    for T, B, ws, name in ri.PATH_TABLE:
        assert rollout.gae_path(T, B, workspace=ws) == name, (T, B, ws)
    for T, B in [(513, 65), (1025, 900)]:
        need = lib.pmenv_gae_workspace(T, B)
        assert need > 0
        assert lib.pmenv_gae_path(T, B, need, 1).decode().startswith("gae_lookback_kernel")
        for nbytes, aligned in [(0, 0), (0, 1), (need - 8, 1), (need, 0)]:      # NULL, too small, misaligned
            assert lib.pmenv_gae_path(T, B, nbytes, aligned).decode() == ri.TILE16
    assert lib.pmenv_gae_workspace(300, 130) == 0 and lib.pmenv_gae_path(300, 130, 0, 0).decode() == ri.TILE16
    assert lib.pmenv_gae_path(0, 5, 0, 1) == b"" and lib.pmenv_gae_path(5, 0, 0, 1) == b""
    for T, B, _ in ri.LOOP_CASES:                                               # the product never loops here
        assert rollout.gae_path(T, B) != ri.LOOP


# ------------------------------------------------------------------------------ metrics
def _metrics(T, B, N, rf, periods=252.0, seed=0):
    ret, val, w = ri.metrics_batch(T, B, N, seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"):
            return ret, val, w, or_metrics(ret, val, w, rf=rf, periods=periods)


def _cls(B, name):
    return [b for b in range(B) if b % ri.KM == ri.MCLASS[name]]


@pytest.mark.parametrize("T,B,N", ri.METRIC_SHAPES)
def test_metric_classes_and_the_oracles_degenerate_patterns(T, B, N):
    ret, val, w, m = _metrics(T, B, N, rf=0.0)
    if B >= ri.KM:
        assert {b % ri.KM for b in range(B)} == set(range(ri.KM))
    assert np.isfinite(ret).all() and np.isfinite(val).all() and (val > 0).all()
    np.testing.assert_allclose(w.astype(np.float64).sum(-1), 1.0, atol=1e-6)
    sharpe, sortino, mdd, turn, final = m.T
    if T == 1:                                   # std(ddof = 1) of one return
        assert np.isnan(sharpe).all()
    else:
        c = _cls(B, "constant")                  # mean > 0 over a zero deviation, no loss, no drawdown
        assert (sharpe[c] == np.inf).all() and (sortino[c] == np.inf).all() and (mdd[c] == 0).all()
        z = _cls(B, "zero")                      # 0 / 0
        assert np.isnan(sharpe[z]).all() and np.isnan(sortino[z]).all() and (mdd[z] == 0).all()
        p = _cls(B, "positive")
        assert np.isfinite(sharpe[p]).all() and (sortino[p] == np.inf).all() and (mdd[p] == 0).all()
    assert (mdd[_cls(B, "rising")] == 0).all()
    f = _cls(B, "falling")
    np.testing.assert_allclose(mdd[f], 1.0 / (1.0 + 0.01 * T) - 1.0, rtol=1e-12)
    np.testing.assert_allclose(mdd[_cls(B, "peak_first")], -0.75, rtol=1e-12)
    for b in _cls(B, "seg_peaks"):               # each wave segment's first day is a new running peak
        firsts = sorted({(T + 1) * k // 4 for k in range(4)})
        run = np.maximum.accumulate(val[:, b])
        assert all(val[t, b] == run[t] and (t == 0 or val[t, b] > run[t - 1]) for t in firsts)
    for b in _cls(B, "alt_weights"):
        np.testing.assert_allclose(turn[b], ri.alt_turnover(w, b), rtol=1e-12)
        assert turn[b] > 0.01
    assert np.array_equal(final, val[-1])


@pytest.mark.parametrize("T,B,N", ri.METRIC_SHAPES)
@pytest.mark.parametrize("rf,periods", ri.METRIC_RATES)
def test_metric_comparisons_are_well_conditioned(T, B, N, rf, periods):
    """Where the GPU test compares sharpe / sortino by value the deviation is far above the
    rounding of the mean (another summation order moves the ratio by ~1e-13); where the deviation
    is zero (the constant and zero classes: one repeated excess return, inexact at rf != 0) the
    restatement's two-pass std is exactly 0 on these inputs and sharpe is sign(mean) x inf (NaN
    for 0 / 0 and for T = 1), the closed form — so the pattern comparison is of exact values."""
    ret, val, w, m = _metrics(T, B, N, rf, periods)
    rfp = (1 + rf) ** (1 / periods) - 1 if rf else 0.0
    x = ret - rfp
    flat = np.array([ri.METRIC_CLASSES[b % ri.KM] in ("constant", "zero") for b in range(B)])
    if T > 1:
        sd = x.std(0, ddof=1)
        assert (sd[~flat] > 1e-6 * np.abs(x).max(0)[~flat]).all() and (sd[flat] == 0.0).all()
        mean = x[0, flat]
        want = np.where(mean == 0.0, np.nan, np.copysign(np.inf, mean))
        assert np.array_equal(m[flat, 0], want, equal_nan=True)
    else:
        assert np.isnan(m[:, 0]).all()
    dn = np.sqrt((np.minimum(x, 0) ** 2).sum(0) / T)
    ok = np.isfinite(m[:, 1])
    assert (dn[ok] > 1e-7).all()
