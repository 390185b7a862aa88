"""The per-episode metrics' restatement and inputs (tests/metrics_env_ref.py), pinned on the
CPU so that test_gpu_metrics_episodes.py cannot pass vacuously: the restatement is the
lockstep oracle where nothing ends, segments are cut as include/pmenv.h states, the done
classes cover what they claim at the tested shapes, and the zero-deviation episodes whose
Sharpe the GPU test leaves out are few and only of the two flat classes."""
import warnings

import numpy as np
import pytest

import metrics_env_ref as mr
import rollout_edge_inputs as ri
from oracle import trajectory_metrics as or_metrics


@pytest.mark.parametrize("rf,periods", ri.METRIC_RATES)
@pytest.mark.parametrize("T,B,N", [(1, 10, 1), (5, 65, 7), (64, 30, 30)])
def test_ref_without_dones_is_the_lockstep_oracle(T, B, N, rf, periods):
    """Exact against the oracle called one column at a time, which is how `ref` calls it: that
    is the comparison that counts. The oracle over the whole batch adds in another order (numpy's
    reduction over axis 0 depends on the array's width), so it is only a sanity check here, at
    rtol 1e-9 and without the Sharpe column: on the zero-deviation classes the two orders can
    give inf on one side and a huge finite number on the other."""
    ret, val, w, _ = mr.batch(T, B, N, seed=3)
    got = mr.ref(ret, val, w, np.zeros((T, B), np.uint8), 123.0, rf, periods)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        # column by column: numpy's order of additions depends on the array's width
        exp = np.concatenate([or_metrics(ret[:, b:b + 1], val[:, b:b + 1], w[:, b:b + 1], rf=rf, periods=periods)
                              for b in range(B)])
        np.testing.assert_allclose(exp[:, 1:], or_metrics(ret, val, w, rf=rf, periods=periods)[:, 1:], rtol=1e-9,
                                   atol=1e-12)
    assert all(len(e) == 1 and e[0][1:] == (1, T) for e in got)
    assert np.array_equal(np.stack([e[0][0] for e in got]), exp, equal_nan=True)


def test_counts_and_spans_of_a_hand_written_case():
    d = np.array([[0, 1, 0, 0, 1, 0],
                  [0, 0, 0, 7, 1, 1],
                  [0, 0, 0, 0, 1, 0],
                  [0, 0, 255, 0, 1, 1],
                  [0, 0, 0, 1, 1, 0]], np.uint8)                  # [T = 5, B = 6]
    want = [[(1, 5)], [(1, 1), (2, 5)], [(1, 4), (5, 5)], [(1, 2), (3, 5)],
            [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5)], [(1, 2), (3, 4), (5, 5)]]
    assert [mr.segments(d[:, b]) for b in range(6)] == want
    T, B, N = 5, 6, 3
    ret, val, w = ri.metrics_batch(T, B, N, seed=1)
    refs = mr.ref(ret, val, w, d, 2.0, 0.04, 252.0)
    out, span, count = mr.dense(refs, 2)
    assert count.tolist() == [1, 2, 2, 2, 5, 3]                   # exact above the cap
    assert span[4].tolist() == [[1, 1], [2, 2]] and span[0].tolist() == [[1, 5], [0, 0]]
    assert np.isnan(out[0, 1]).all() and not np.isnan(out[4, :, 4]).any()


def test_terminal_row_belongs_to_the_ending_episode():
    """Env 0 ends an episode with step 3: values / weights row 3 are that episode's last row
    (its final value, a drawdown against its own peak, its last turnover term); the next
    episode starts from init_value and e0 and sees nothing of row 3."""
    T, B, N = 6, 1, 4
    ret, val, w = ri.metrics_batch(T, B, N, seed=2)
    d = np.zeros((T, B), np.uint8)
    d[2, 0] = 1
    base = mr.ref(ret, val, w, d, 1.5, 0.0, 252.0)[0]
    assert [(f, l) for _, f, l in base] == [(1, 3), (4, 6)]
    assert base[0][0][4] == val[3, 0] and base[1][0][4] == val[6, 0]
    v2, w2 = val.copy(), w.copy()
    v2[3, 0] = 1e-3                                               # a crash on the terminal row
    w2[3, 0] = np.roll(w[3, 0], 1)
    got = mr.ref(ret, v2, w2, d, 1.5, 0.0, 252.0)[0]
    assert got[0][0][2] < -0.99 and got[0][0][4] == 1e-3 and got[0][0][3] != base[0][0][3]
    assert np.array_equal(got[1][0], base[1][0], equal_nan=True)
    # the second episode's path starts at init_value, its weights at e0
    e0 = np.eye(N, dtype=np.float32)[0]
    turn = np.abs(np.diff(np.concatenate([e0[None], w[4:7, 0]]).astype(np.float64), axis=0)).sum() / 3
    np.testing.assert_allclose(base[1][0][3], turn, rtol=1e-14)
    path = np.concatenate([[1.5], val[4:7, 0]])
    assert base[1][0][2] == min(0.0, (path / np.maximum.accumulate(path) - 1).min())


@pytest.mark.parametrize("T,B,N", mr.ALL_SHAPES)
def test_done_classes_cover_what_they_claim(T, B, N):
    _, _, _, d = mr.case(T, B, N)
    assert d.shape == (T, B) and d.dtype == np.uint8
    cls = np.arange(B) % mr.KD
    if B >= 90:                                  # every (done class, value class) pair
        assert {(b % mr.KD, b % ri.KM) for b in range(B)} == {(i, j) for i in range(mr.KD) for j in range(ri.KM)}
    cnt = (d != 0).sum(0)
    for name, want in [("none", 0), ("every", T), ("last_only", 1), ("first_only", 1), ("single", 1)]:
        assert (cnt[cls == mr.DCLASS[name]] == want).all(), name
    if (cls == mr.DCLASS["last_only"]).any():
        assert (d[T - 1, cls == mr.DCLASS["last_only"]] != 0).all()
    if (cls == mr.DCLASS["first_only"]).any():
        assert (d[0, cls == mr.DCLASS["first_only"]] != 0).all()
    assert (cnt[cls == mr.DCLASS["pair"]] == min(2, T)).all()
    if B >= 9 * T:                               # a boundary after every row, alone and next to another
        for name in ("single", "pair"):
            rows = set(np.flatnonzero((d[:, cls == mr.DCLASS[name]] != 0).any(1)).tolist())
            assert rows == set(range(T)), name
    byt = d[:, cls == mr.DCLASS["bytes"]]
    assert set(np.unique(byt).tolist()) <= {0, 2, 128, 255}
    if T * B >= 9 * 64:
        assert {2, 128, 255} <= set(np.unique(byt).tolist())
        rnd = cnt[cls == mr.DCLASS["random"]]
        assert rnd.min() < rnd.max()
    others = d[:, cls != mr.DCLASS["bytes"]]
    assert set(np.unique(others).tolist()) <= {0, 1}


@pytest.mark.parametrize("rf,periods", ri.METRIC_RATES)
@pytest.mark.parametrize("T,B,N", mr.ALL_SHAPES)
def test_sharpe_comparison_rule_and_its_cap(T, B, N, rf, periods):
    """Which zero-deviation episodes have a restatement Sharpe of exactly +-inf or NaN: only
    those enter the GPU pattern comparison of Sharpe; the episodes left out are of the two flat
    classes only, so never more than those classes' episodes, and their other four fields stay
    compared. That cap holds by the rule's construction; what bounds the rule from the other side
    is arithmetic. With rf = 0 the repeated excess return is 0 or 2^-7, every partial sum is exact,
    the two-pass std is exactly 0 and no episode at all may be left out. With rf != 0 the mean of
    one or two equal numbers is still exact, so every flat episode of n <= 2 steps must be kept;
    only longer ones may round. Everywhere else a finite restatement Sharpe rests on a deviation
    far above the rounding of the mean."""
    ret, val, w, d = mr.case(T, B, N)
    refs = mr.case_ref(T, B, N, rf, periods)
    K = T + 1
    keep = mr.sharpe_compared(refs, K)
    out, span, count = mr.dense(refs, K)
    assert (count <= K).all()
    stored = np.arange(K)[None, :] < count[:, None]
    flat = np.array([ri.METRIC_CLASSES[b % ri.KM] in mr.FLAT for b in range(B)])
    left_out = stored & ~keep
    assert not left_out[~flat].any()
    assert left_out.sum() <= stored[flat].sum()
    if rf == 0.0:
        assert not left_out.any()
    steps = span[..., 1] - span[..., 0] + 1
    assert not (left_out & (steps <= 2)).any()
    if (stored[flat] & (steps[flat] <= 2)).any():
        assert (keep & stored)[flat].any()
    rfp = (1 + rf) ** (1 / periods) - 1 if rf else 0.0
    for b in range(B):
        for k in range(count[b]):
            first, last = span[b, k]
            x = ret[first - 1:last, b] - rfp
            sh = out[b, k, 0]
            if flat[b]:
                assert (x == x[0]).all()
                if keep[b, k]:                   # the closed form: sign(mean) x inf, NaN for 0 / 0 and n = 1
                    want = np.nan if (x.size == 1 or x[0] == 0.0) else np.copysign(np.inf, x[0])
                    assert np.array_equal(sh, want, equal_nan=True), (b, k)
            elif x.size > 1:
                assert np.isfinite(sh) and x.std(ddof=1) > 1e-6 * np.abs(x).max(), (b, k)
            else:
                assert np.isnan(sh)
