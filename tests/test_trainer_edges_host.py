"""The batched reward's edge catalogue (trainer_edge_inputs.py) on the CPU: no GPU needed.

  * every case through the oracle and through an f64 torch-autograd restatement of the
    reference's reward (agent/pg/pg.py:40-82, written out below): NaN / +inf / -inf / finite
    classes equal, finite values at the trainer's tolerances;
  * the properties the cases exist for, in the reference alone: the threshold flags, the
    marker row's weight in the reward, and that a planted inf / NaN stays in its row under
    `returns` / `log_returns` (what the GPU containment assertion rests on);
  * pmenv_batch_reward_path (host only: the library loads without a device) against
    trainer_edge_inputs.path_rules over B 1..130 x N 1..520 and the fold shapes, with the
    thresholds pinned by literal strings;
  * the catalogue reaches every forward and backward kernel and every partial count, by name.
"""
import warnings

import numpy as np
import pytest
import torch

import trainer_edge_inputs as ti
from oracle import batch_reward as or_batch_reward

F64 = torch.float64


# ---------------------------------------------------------------- the reference, restated
def autograd_reward(case, kind, norm, scale):
    """pg.py:40-82 in f64 with COMISSION = 0: normalise by softmax over the assets when the
    weights do not sum to 1 (isclose, atol 1e-6) or hold a negative entry - decided over the
    whole tensor (the reference), per row, or never; value = sum_n v (w p); ret = value / v;
    reward = mean(ret), mean(log ret) or mean(ret) / std(ret), times scale.
    Returns (R, ret [B], dR/da [B, N]) as f64 numpy."""
    B, N = case.a.shape
    a = torch.tensor(case.a, dtype=F64).reshape(B, N, 1).requires_grad_(True)
    v = torch.tensor(case.v, dtype=F64).reshape(B, 1, 1)
    p = torch.tensor(case.p, dtype=F64).reshape(B, N, 1)
    one = torch.tensor(1.0, dtype=F64)
    w = a
    if norm == "global_or":
        if not torch.isclose(torch.sum(a), one, atol=1e-6) or torch.min(a) < 0:
            w = torch.softmax(a, dim=1)
    elif norm == "softmax":                                  # (the tests' own: every row normalised)
        w = torch.softmax(a, dim=1)
    elif norm == "row_or":
        d = a.detach()
        mn = d.min(dim=1, keepdim=True).values
        soft = ~torch.isclose(d.sum(dim=1, keepdim=True), one, atol=1e-6) | (mn < 0) | torch.isnan(mn)
        w = torch.where(soft, torch.softmax(a, dim=1), a)
    value = torch.sum(v * (w * p), dim=1, keepdim=True)
    ret = value / v
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # std of one element
        if kind == "returns":
            r = torch.mean(ret * scale)
        elif kind == "log_returns":
            r = torch.mean(torch.log(ret) * scale)
        else:
            r = torch.mean(ret) / torch.std(ret) * scale
    r.backward()
    return float(r.detach()), ret.detach().reshape(B).numpy(), a.grad.reshape(B, N).numpy()


def check_against_autograd(case, kind, norm, scale=None):
    scale = case.scale if scale is None else scale
    what = f"{case.name} {kind} {norm}"
    with np.errstate(all="ignore"):
        R, oret, og = or_batch_reward(case.a, case.v, case.p, reward=kind, norm=norm, scale=scale)
        tR, tret, tg = autograd_reward(case, kind, norm, scale)
        assert ti.classes(R) == ti.classes(tR), (what, R, tR)
        assert np.isclose(R, tR, rtol=1e-6, atol=1e-12, equal_nan=True), (what, R, tR)
        ti.compare_ret(oret, tret.astype(np.float32), what)
        ti.compare_grad(og, tg.astype(np.float32), what)
    return R, oret, og


def all_cases():
    for N in ti.FORM_NS:
        yield from ti.shape_cases(N)
    for B in ti.EDGE_BS:
        yield from ti.n_edge_cases(B)
    for B, N in ti.THRESHOLD_SHAPES:
        yield from ti.threshold_cases(B, N)
    for B, N in ti.VALUE_SHAPES:
        yield from ti.value_cases(B, N)
    for N in ti.FORM_NS:
        yield ti.sharpe_single_row_case(N)


def catalogue_shapes():
    s = {(B, N) for N in ti.FORM_NS for B in ti.SHAPE_BS} | {(B, N) for B in ti.EDGE_BS for N in ti.EDGE_NS}
    s |= set(ti.THRESHOLD_SHAPES) | set(ti.VALUE_SHAPES) | {(1, N) for N in ti.FORM_NS}
    s |= {ti.fold_shape(f, k) for f in ti.FOLD_FORMS for k in ti.FOLD_PARTS}
    return s


# ---------------------------------------------------------------- oracle == autograd
@pytest.mark.parametrize("N", ti.FORM_NS)
def test_shape_cases_oracle_matches_autograd(N):
    for i, case in enumerate(ti.shape_cases(N)):
        for kind in case.kinds:
            for norm in case.norms:
                check_against_autograd(case, kind, norm, scale=1000.0 if i % 2 else 1.0)


@pytest.mark.parametrize("B", ti.EDGE_BS)
def test_n_edge_cases_oracle_matches_autograd(B):
    for case in ti.n_edge_cases(B):
        for kind in case.kinds:
            for norm in case.norms:
                check_against_autograd(case, kind, norm)


@pytest.mark.parametrize("form", sorted(ti.FOLD_FORMS))
@pytest.mark.parametrize("parts", ti.FOLD_PARTS)
def test_fold_cases_oracle_matches_autograd_and_the_marker_row_weighs(form, parts):
    """A fold that loses or doubles the marker row's term (the batch size it divides by is
    the host's B either way) moves the reward by at least 10 x the reward tolerance, for each
    kind: no partial can go missing under the GPU test's reward tolerance. For Sharpe the
    lost row leaves the count, mean and M2 of the merged records."""
    B, _ = ti.fold_shape(form, parts)
    for i, (name, row) in enumerate(ti.fold_markers(form, parts).items()):
        norm = ti.NORMS[i % 3]
        case = ti.fold_case(form, parts, row, norm)
        kind = ti.KINDS[i % 3]
        _, oret, _ = check_against_autograd(case, kind, norm)                    # one kind per marker: 2 M elements
        x = oret.astype(np.float64)
        assert x[row] == 2.0 or abs(x[row] - 2.0) < 1e-6
        assert np.abs(np.delete(x, row) - 1.0).max() < 0.1
        for kind in ti.KINDS:
            def reward(xs):
                if kind == "returns":
                    return xs.sum() / B
                if kind == "log_returns":
                    return np.log(xs).sum() / B
                return xs.mean() / np.sqrt(((xs - xs.mean()) ** 2).sum() / (B - 1))
            R = reward(x)
            tol = 1e-6 * abs(R) + 1e-12
            lost, doubled = reward(np.delete(x, row)), reward(np.append(x, x[row]))
            assert abs(lost - R) >= 10 * tol, (name, kind, R, lost)
            assert abs(doubled - R) >= 10 * tol, (name, kind, R, doubled)


@pytest.mark.parametrize("B,N", ti.THRESHOLD_SHAPES)
def test_threshold_cases_flags_and_flip(B, N):
    """The batch (global_or) and the rows (row_or) take the side of the rule they were built
    for: raw returns are bit-equal to norm = none's, softmax ones to a batch that normalises,
    and the two differ by far more than the tolerances."""
    want_rows = ti.threshold_row_flags(B)
    for case in ti.threshold_cases(B, N):
        for kind in case.kinds:
            for norm in case.norms:
                check_against_autograd(case, kind, norm)
        _, raw, _ = or_batch_reward(case.a, case.v, case.p, reward="returns", norm="none")
        rows = case.name.startswith("thr_rows")
        norm = "row_or" if rows else "global_or"
        flags = ti.expected_flags(case.a, norm)
        if rows:
            assert np.array_equal(flags, want_rows), case.name
        else:
            want = dict((c[0], c[3]) for c in ti.ROW_CLASSES)[case.name.split("_", 2)[2].rsplit("_", 1)[0]]
            assert flags.all() == want and flags.any() == want, case.name
        R, got, _ = or_batch_reward(case.a, case.v, case.p, reward="returns", norm=norm)
        if not rows:                                         # raw: the rows share one unit of weight
            assert (R > 0.8) if want else (R < 0.2), (case.name, R)
        _, tsoft, _ = autograd_reward(case, "returns", "softmax", 1.0)
        assert np.array_equal(got[~flags], raw[~flags]), case.name
        np.testing.assert_allclose(got[flags], tsoft[flags], rtol=1e-7)
        # ... and a wrong decision would show in the returns as well: the candidates are apart
        assert (np.abs(got[flags] - raw[flags]) > 16 * np.spacing(np.abs(raw[flags]))).all(), case.name


@pytest.mark.parametrize("B,N", ti.VALUE_SHAPES)
def test_value_cases_oracle_matches_autograd_and_poison_stays_in_its_row(B, N):
    for case in ti.value_cases(B, N):
        clean = np.setdiff1d(np.arange(B), case.planted)
        for kind in case.kinds:
            for norm in case.norms:
                _, _, og = check_against_autograd(case, kind, norm)
                if kind != "sharpe_ratio":
                    bad = clean[~np.isfinite(og[clean]).all(1)]
                    assert bad.size == 0, f"{case.name} {kind} {norm}: rows {bad} lost a finite gradient"
        # the planted rows are not all lost either: something non-finite does come out
        if case.planted and "returns" in case.kinds:
            _, _, og = or_batch_reward(case.a, case.v, case.p, reward="returns", norm="none")
            _, _, og2 = or_batch_reward(case.a, case.v, case.p, reward="log_returns", norm="global_or")
            assert not (np.isfinite(og).all() and np.isfinite(og2).all()), case.name


@pytest.mark.parametrize("N", ti.FORM_NS)
def test_sharpe_of_one_row_is_nan(N):
    case = ti.sharpe_single_row_case(N)
    for norm in case.norms:
        R, _, og = check_against_autograd(case, "sharpe_ratio", norm)
        assert np.isnan(R) and np.isnan(og).all()


# ---------------------------------------------------------------- the form by name
ANCHORS = {
    (64, 30): "batch_reward_small_kernel<8> | batch_reward_grad_quad_kernel<8> | parts=1",
    (64, 32): "batch_reward_small_kernel<8> | batch_reward_grad_quad_kernel<8> | parts=1",
    (64, 33): "batch_reward_small_kernel<16> | batch_reward_grad_quad_kernel<16> | parts=1",
    (64, 64): "batch_reward_small_kernel<16> | batch_reward_grad_quad_kernel<16> | parts=1",
    (64, 65): "batch_reward_rows_kernel<2> | batch_reward_grad_kernel<2> | parts=4",
    (65, 32): "batch_reward_rows_quad_kernel<8> | batch_reward_grad_quad_kernel<8> | parts=2",
    (65, 33): "batch_reward_rows_quad_kernel<16> | batch_reward_grad_quad_kernel<16> | parts=2",
    (65, 64): "batch_reward_rows_quad_kernel<16> | batch_reward_grad_quad_kernel<16> | parts=2",
    (65, 65): "batch_reward_rows_kernel<2> | batch_reward_grad_kernel<2> | parts=5",
    (16, 128): "batch_reward_rows_kernel<2> | batch_reward_grad_kernel<2> | parts=1",
    (17, 129): "batch_reward_rows_kernel<4> | batch_reward_grad_kernel<4> | parts=2",
    (3, 256): "batch_reward_rows_kernel<4> | batch_reward_grad_kernel<4> | parts=1",
    (3, 257): "batch_reward_rows_kernel<8> | batch_reward_grad_kernel<8> | parts=1",
    (3, 512): "batch_reward_rows_kernel<8> | batch_reward_grad_kernel<8> | parts=1",
    (3, 513): "batch_reward_rows_kernel<0> | batch_reward_grad_kernel<0> | parts=1",
    (131073, 4): "batch_reward_rows_quad_kernel<8> | batch_reward_grad_quad_kernel<8> | parts=2049",
    (32769, 65): "batch_reward_rows_kernel<2> | batch_reward_grad_kernel<2> | parts=2049",
}


def lib_path(B, N):
    from pmenv import _abi
    return _abi.load().pmenv_batch_reward_path(B, N).decode()


def test_batch_reward_path_matches_the_rules():
    for (B, N), want in ANCHORS.items():
        assert lib_path(B, N) == want == ti.path_rules(B, N), (B, N)
    for B in range(1, 131):
        for N in range(1, 521):
            assert lib_path(B, N) == ti.path_rules(B, N), (B, N)
    for B, N in sorted(catalogue_shapes()):
        assert lib_path(B, N) == ti.path_rules(B, N), (B, N)
    for B, N in ((0, 5), (5, 0), (-1, 30), (30, -1), (0, 0)):
        assert lib_path(B, N) == "", (B, N)


def test_catalogue_reaches_every_kernel_and_partial_count():
    fwd, bwd, parts = set(), set(), {"quad": set(), "wave": set()}
    for B, N in catalogue_shapes():
        f, b, k = ti.parse_path(lib_path(B, N))
        fwd.add(f)
        bwd.add(b)
        parts["quad" if N <= 64 else "wave"].add(k)
    assert fwd == {"batch_reward_small_kernel<8>", "batch_reward_small_kernel<16>",
                   "batch_reward_rows_quad_kernel<8>", "batch_reward_rows_quad_kernel<16>",
                   "batch_reward_rows_kernel<2>", "batch_reward_rows_kernel<4>",
                   "batch_reward_rows_kernel<8>", "batch_reward_rows_kernel<0>"}
    assert bwd == {"batch_reward_grad_quad_kernel<8>", "batch_reward_grad_quad_kernel<16>",
                   "batch_reward_grad_kernel<2>", "batch_reward_grad_kernel<4>",
                   "batch_reward_grad_kernel<8>", "batch_reward_grad_kernel<0>"}
    for form in ("quad", "wave"):
        assert set(ti.FOLD_PARTS) <= parts[form], (form, sorted(parts[form]))
        N, rows = ti.FOLD_FORMS[form]
        for k in ti.FOLD_PARTS:
            B, _ = ti.fold_shape(form, k)
            f, _, got = ti.parse_path(lib_path(B, N))
            assert got == k and -(-B // rows) == k and "small" not in f, (form, k, B)
    # each form's N in FORM_NS is the form the GPU tests name it by
    forms = [ti.parse_path(lib_path(65, N))[1] for N in ti.FORM_NS]
    assert forms == ["batch_reward_grad_quad_kernel<8>"] * 2 + ["batch_reward_grad_quad_kernel<16>"] * 2 + [
        "batch_reward_grad_kernel<2>", "batch_reward_grad_kernel<4>", "batch_reward_grad_kernel<8>",
        "batch_reward_grad_kernel<0>"]
