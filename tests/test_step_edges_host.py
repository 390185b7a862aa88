"""The edge generator's preconditions (tests/edge_inputs.py), pinned against the CPU
restatement alone for every (shape, config) test_gpu_step_edges.py runs. They are what makes
the project's parity tolerances applicable to these inputs: conditions on the inputs — if
one fails for a shape, the inputs change, not the condition."""
import numpy as np
import pytest

import edge_inputs as ei


def _unique_runs():
    seen, out = set(), []
    for shape, cid, kw in ei.finite_cases():
        _, _, mode, N, W, F, B, _ = shape
        key = (mode, N, W, F, B, cid)
        if key not in seen:
            seen.add(key)
            out.append(pytest.param(shape, kw, id=f"{mode}-n{N}-w{W}-f{F}-b{B}-{cid}"))
    return out


@pytest.mark.parametrize("shape,kw", _unique_runs())
def test_edge_batch_preconditions(shape, kw):
    _, _, mode, N, W, F, B, _ = shape
    cfg = ei.env_config(shape, kw)
    T = ei.steps(W)
    bt = ei.batch(B, N, W, T, F)
    resets = ei.reset_masks(B, W)
    # every float32 action row's float64 sum is far from the isclose threshold: another
    # summation order (a few ulp of 1) cannot flip the normalisation decision
    assert ei.isclose_margin(bt["act"]) >= 1e-6
    ref = ei.oracle_run(cfg, bt, mode, resets)
    since = np.zeros(B, int)                   # steps since the env's last reset
    for t in range(T):
        if t in resets:
            since[resets[t]] = 0
        since += 1
        r, ret, w, v = ref["r"][t], ref["ret"][t], ref["w"][t], ref["value"][t]
        first = since == 1
        if cfg.reward == "sharpe_ratio":       # numpy's std(ddof=1) of one return: NaN, as documented
            assert np.all(np.isnan(r[first])) and np.all(np.isfinite(r[~first])), f"step {t}"
        else:
            assert np.all(np.isfinite(r)), f"step {t}: reward"
        assert np.all(np.isfinite(ret)) and np.all(np.isfinite(v)) and np.all(v > 0), f"step {t}"
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(ref["obs"][t])), f"step {t}"
        # no cancellation in the value: sum |w'| stays O(1)
        assert np.abs(w.astype(np.float64)).sum(-1).max() <= 4.0, f"step {t}: sum |w'|"
        assert np.all(np.isfinite(ref["sa"][t])) and np.all(np.isfinite(ref["sb"][t]))
        if cfg.reward == "diff_sharpe":
            # the variance is never within a factor 10 of the 1e-12 switch after an env's
            # first step (where it is exactly 0 on both sides): the branch cannot differ
            var = ref["sb"][t] - ref["sa"][t] ** 2
            assert np.all((var > 1e-11) | (var < 1e-13)), f"step {t}: var {var.min():.3e}"


def test_edge_classes_cover_both_norm_outcomes():
    """The class table's claim, checked on the generator's own rows: which classes AND / OR
    mode normalise (so a wave always holds envs on both sides of the decision)."""
    rng = np.random.default_rng(1)
    for N in (30, 70):          # (at N = 5 a simplex entry can exceed the 0.2 / 0.3 the classes take off)
        a = ei.actions(rng, ei.K, N, 0).astype(np.float64)      # env b = class b
        not_close = np.abs(a.sum(-1) - 1.0) > ei.ISCLOSE
        negative = a.min(-1) < 0
        assert list(not_close & negative) == [c in (3, 6, 8) for c in range(ei.K)]
        assert list(not_close | negative) == [c not in (0, 4, 5) for c in range(ei.K)]


def test_edge_series_carries_its_relatives():
    """The advance legs' close series is finite and positive, and the dead asset's falls and the
    jumps are in it."""
    B, N, W = ei.B_EDGE, 30, 4
    bt = ei.batch(B, N, W, ei.steps(W))
    c = bt["ser"][..., 3].astype(np.float64)
    assert np.all(np.isfinite(bt["ser"])) and np.all(bt["ser"] > 0)
    y = c[W:] / c[W - 1:-1]
    np.testing.assert_allclose(y[4::8, ::7, 3], 2.0 ** -8, rtol=1e-6)
    np.testing.assert_allclose(y[0::8, 3::11, 2], 30.0, rtol=1e-6)
    assert np.all(bt["y"][:, ::7, 3] == 0) and np.all(bt["y"][:, 3::11, 2] == 30)
