"""Hand-built inputs for the batched PG / A2C reward (csrc/trainer.h), shared by the CPU tests
(test_trainer_edges_host.py) and the GPU tests (test_gpu_trainer_edges.py). numpy only.

Every case is a `Case`: a [B, N], v_prev [B], p [B, N] (f32), the reward kinds and norm modes
it is run under, the `scale`, what it is for, the rows something was planted in (`planted`:
every other row must keep a finite gradient under `returns` / `log_returns`, where a row's
dR/dret depends on that row alone) and, for the fold cases, the marker row.

  shape_cases / n_edge_cases   every kernel form either side of its dispatch thresholds and of
                               the record's row counts; rows cycle random-normal, simplex and
                               negative-entry, so neighbours in one quad-wave and one 16-row
                               block fall in different classes
  fold_case                    255 ... 2049 partial records in the quad and the wave form, one
                               marker row of return 2 among returns near 1
  threshold_cases              sums of multiples of 2^-24 (exact in f64 in any order) that sit
                               2^-17 (raw) or 2^-16 (softmax) off 1, and min = 0 / -2^-24 / -0.0
  value_cases                  inf / NaN / 0 in p, v_prev and a

`path_rules` restates the dispatch of pmenv_batch_reward_forward / _backward, and
`expected_flags` the normalisation decision per row.
"""
import collections

import numpy as np

KINDS = ("log_returns", "returns", "sharpe_ratio")
NORMS = ("global_or", "row_or", "none")
FORM_NS = (5, 30, 33, 64, 65, 129, 257, 513)                 # one N per kernel form
SHAPE_BS = (1, 2, 15, 16, 17, 31, 33, 47, 49, 63, 64, 65, 127, 128, 129)
EDGE_BS = (3, 65)
EDGE_NS = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 577, 700)
FOLD_PARTS = (255, 256, 257, 1023, 1024, 1025, 2049)
FOLD_FORMS = {"quad": (4, 64), "wave": (65, 16)}             # N, rows per partial record
THRESHOLD_SHAPES = ((8, 6), (40, 40), (70, 30), (70, 33), (37, 65), (33, 129), (20, 257), (20, 513))
VALUE_SHAPES = tuple((B, N) for B in (9, 70) for N in (30, 33, 65, 513))
ISCLOSE = 1e-6 + 1e-5                                        # torch.isclose(sum, 1, atol=1e-6): rtol 1e-5 of 1
U = 2.0 ** -24

Case = collections.namedtuple("Case", "name a v p kinds norms scale what planted marker")


def _case(name, a, v, p, what, kinds=KINDS, norms=NORMS, scale=1.0, planted=(), marker=None):
    a, v, p = (np.ascontiguousarray(x, dtype=np.float32) for x in (a, v, p))
    assert a.ndim == 2 and p.shape == a.shape and v.shape == (a.shape[0],)
    return Case(name, a, v, p, tuple(kinds), tuple(norms), float(scale), what, tuple(sorted(planted)), marker)


# ---------------------------------------------------------------- the dispatch, restated
def path_rules(B, N):
    """What pmenv_batch_reward_path(B, N) must say: the forward's row kernel, the backward
    kernel and the number of partial records the fold reads."""
    if B < 1 or N < 1:
        return ""
    if N <= 64:                                               # four lanes per row, 64 rows per record
        epl = 8 if N <= 32 else 16
        fwd = "batch_reward_small_kernel" if B <= 64 else "batch_reward_rows_quad_kernel"
        return f"{fwd}<{epl}> | batch_reward_grad_quad_kernel<{epl}> | parts={-(-B // 64)}"
    epl = 2 if N <= 128 else 4 if N <= 256 else 8 if N <= 512 else 0      # a wave per row, 16 rows per record
    return f"batch_reward_rows_kernel<{epl}> | batch_reward_grad_kernel<{epl}> | parts={-(-B // 16)}"


def parse_path(text):
    fwd, bwd, parts = text.split(" | ")
    return fwd, bwd, int(parts.split("=")[1])


def expected_flags(a, norm):
    """The per-row normalisation decision (work[5B + b]) in f64: pg.py:52 over the whole batch
    (global_or), the same rule per row (row_or), never (none). NaN anywhere makes the sum NaN,
    so the row (or batch) normalises."""
    a = np.asarray(a, np.float64)
    B = a.shape[0]
    with np.errstate(invalid="ignore"):
        if norm == "none":
            return np.zeros(B, bool)
        if norm == "global_or":
            s, mn = a.sum(), a.min()
            return np.full(B, bool(not (abs(s - 1.0) <= ISCLOSE) or mn < 0.0))
        s, mn = a.sum(1), a.min(1)
        return ~(np.abs(s - 1.0) <= ISCLOSE) | (mn < 0.0) | np.isnan(mn)


# ---------------------------------------------------------------- shapes
def _mixed_rows(rng, B, N):
    """Row b is random normal (b % 3 == 0), on the simplex (1) or a simplex row with its first
    entry negated (2)."""
    a = rng.standard_normal((B, N)).astype(np.float32)
    s = np.abs(rng.standard_normal((B, N))).astype(np.float32) + np.float32(1e-3)
    s /= s.sum(1, keepdims=True, dtype=np.float32)
    s[2::3, 0] *= -1
    a[1::3] = s[1::3]
    a[2::3] = s[2::3]
    return a


def _market(rng, B, N):
    v = (25000.0 * np.exp(0.1 * rng.standard_normal(B))).astype(np.float32)
    p = (1.0 + 0.01 * rng.standard_normal((B, N))).astype(np.float32)
    return v, p


def shape_case(B, N):
    rng = np.random.default_rng(1000 * B + N)
    v, p = _market(rng, B, N)
    return _case(f"shape_{B}x{N}", _mixed_rows(rng, B, N), v, p, "dispatch threshold / record row count")


def shape_cases(N):
    return [shape_case(B, N) for B in SHAPE_BS]


def n_edge_cases(B):
    return [shape_case(B, N) for N in EDGE_NS]


# ---------------------------------------------------------------- fold trip count
def fold_shape(form, parts):
    """(B, N) that gives `parts` partial records: a full last record at 256 and 1024, one
    row in it at 257, 1023, 1025 and 2049, a part-filled one at 255."""
    N, rows = FOLD_FORMS[form]
    last = {255: rows * 27 // 64 + 1, 256: rows, 1024: rows}.get(parts, 1)
    return rows * (parts - 1) + last, N


def fold_markers(form, parts):
    """name -> row: row 0, the last row, the first and last row of the last partial and the
    rows either side of the start of partial 1024 (the outer loop's second trip)."""
    B, _ = fold_shape(form, parts)
    rows = FOLD_FORMS[form][1]
    m = {"row0": 0, "last_row": B - 1, "last_part_first": rows * (parts - 1)}
    if parts > 1024:
        m["before_part_1024"] = rows * 1024 - 1
        m["first_of_part_1024"] = rows * 1024
    out, seen = {}, set()
    for k, r in m.items():
        if r not in seen:
            out[k] = r
            seen.add(r)
    return out


_FOLD_BASE = {}


def fold_case(form, parts, marker_row, norm):
    """Simplex rows (so raw and softmax returns are both near 1) and p = 2 along the marker
    row: its return is 2 under either normalisation."""
    B, N = fold_shape(form, parts)
    if (form, parts) not in _FOLD_BASE:
        _FOLD_BASE.clear()                                   # one shape's arrays at a time
        rng = np.random.default_rng(7 * parts + N)
        a = np.abs(rng.standard_normal((B, N))).astype(np.float32) + np.float32(1e-3)
        a /= a.sum(1, keepdims=True, dtype=np.float32)
        _FOLD_BASE[(form, parts)] = (a,) + _market(rng, B, N)
    a, v, p = _FOLD_BASE[(form, parts)]
    p = p.copy()
    p[marker_row] = 2.0
    return _case(f"fold_{form}_{parts}_m{marker_row}", a, v, p, "fold trip count and k < nblk guards",
                 norms=(norm,), marker=marker_row)


# ---------------------------------------------------------------- normalisation threshold
def _units(rng, n, total):
    """n positive integers that sum to `total`, uneven (so raw and softmax weights differ)."""
    w = rng.random(n) ** 2 + 0.02
    k = np.maximum(np.floor(w / w.sum() * total).astype(np.int64), 1)
    k[int(np.argmax(k))] += total - int(k.sum())
    assert k.sum() == total and k.min() >= 1
    return k


ROW_CLASSES = (            # name, units off 2^24, min variant, normalises
    ("in_plus", 2 ** 7, None, False), ("out_plus", 2 ** 8, None, True),
    ("in_minus", -2 ** 7, None, False), ("out_minus", -2 ** 8, None, True),
    ("min_zero", 0, "zero", False), ("min_negative", 0, "neg", True), ("min_negative_zero", 0, "negzero", False))


def _threshold_block(rng, n, delta_units, variant):
    """n f32 values, each a multiple of 2^-24 below 1, summing to 1 + delta_units 2^-24 exactly."""
    k = _units(rng, n, 2 ** 24 + delta_units).astype(np.float64)
    j = int(np.argmin(k))
    big = int(np.argmax(k))
    if variant is not None and n > 1:
        k[big] += k[j] + (1 if variant == "neg" else 0)
        k[j] = {"zero": 0.0, "neg": -1.0, "negzero": -0.0}[variant]
    x = (k * U).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), k * U)       # exact in f32
    assert x.astype(np.float64).sum() == 1.0 + delta_units * U
    return x


def threshold_cases(B, N):
    """Seven global_or batches (the batch sum / min on either side of the rule) and one row_or
    batch whose rows cycle through the seven classes (row b: ROW_CLASSES[b % 7])."""
    rng = np.random.default_rng(31 * B + N)
    v = (25000.0 * np.exp(0.1 * rng.standard_normal(B))).astype(np.float32)
    p = (1.0 + 0.25 * rng.uniform(-1, 1, (B, N))).astype(np.float32)
    out = []
    for name, du, variant, _ in ROW_CLASSES:
        a = _threshold_block(rng, B * N, du, variant).reshape(B, N)
        out.append(_case(f"thr_global_{name}_{B}x{N}", a, v, p, "batch sum / min at the isclose threshold"))
    a = np.stack([_threshold_block(rng, N, *ROW_CLASSES[b % 7][1:3]) for b in range(B)])
    out.append(_case(f"thr_rows_{B}x{N}", a, v, p, "row sums / mins at the isclose threshold"))
    return out


def threshold_row_flags(B):
    return np.array([ROW_CLASSES[b % 7][3] for b in range(B)])


# ---------------------------------------------------------------- values
def value_cases(B, N):
    """Non-finite and zero values on single rows. Rows r0 .. r0 + 8 carry them: r0 = 0 at
    B = 9, r0 = 60 at B = 70 (either side of the quad form's 64-row block)."""
    rng = np.random.default_rng(77 * B + N)
    v, p = _market(rng, B, N)
    a = _mixed_rows(rng, B, N)
    r0 = 0 if B < 69 else 60
    out = []

    q = p.copy()
    q[r0 + 3, 0] = np.inf                                     # the 16-B loads of row r0 + 2 run on into these
    q[r0 + 7, 1] = np.nan                                     # ... and those of row r0 + 6 into this
    out.append(_case(f"val_p_next_rows_{B}x{N}", a, v, q, "inf / NaN in the next rows' p stays out of a row",
                     planted=(r0 + 3, r0 + 7)))

    w = v.copy()
    w[r0], w[r0 + 2], w[r0 + 4], w[r0 + 6] = 0.0, np.inf, 1e-40, 1e30
    out.append(_case(f"val_v_prev_{B}x{N}", a, w, p, "v_prev = 0, inf, 1e-40, 1e30 on single rows",
                     planted=(r0, r0 + 2)))

    x = a.copy()
    x[r0 + 1, N // 2] = -np.inf
    x[r0 + 3] = 80.0
    x[r0 + 3, N - 1] = -80.0
    x[r0 + 5, 1] = np.inf
    x[r0 + 7] = -np.inf
    x[r0 + 8] = np.nan
    out.append(_case(f"val_a_{B}x{N}", x, v, p, "-inf, +-80, +inf entries; an all -inf row; a NaN row",
                     planted=(r0 + 1, r0 + 3, r0 + 5, r0 + 7, r0 + 8)))

    q = p.copy()
    q[r0 + 2, 4] = 0.0
    q[r0 + 5] = 0.0
    out.append(_case(f"val_p_zero_{B}x{N}", a, v, q, "p = 0 for one asset and for a whole row",
                     planted=(r0 + 5,)))

    x = a.copy()
    x[r0 + 1] = -np.abs(a[r0 + 1])
    out.append(_case(f"val_negative_return_{B}x{N}", x, v, p, "log of a negative return (norm = none)",
                     kinds=("log_returns",), norms=("none",)))
    return out


def sharpe_single_row_case(N):
    rng = np.random.default_rng(N)
    v, p = _market(rng, 1, N)
    return _case(f"val_sharpe_1x{N}", _mixed_rows(rng, 1, N), v, p, "B = 1 under Sharpe: std of one return",
                 kinds=("sharpe_ratio",))


# ---------------------------------------------------------------- comparisons
def classes(x):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, per element."""
    x = np.asarray(x)
    return np.where(np.isnan(x), 1, np.where(np.isposinf(x), 2, np.where(np.isneginf(x), 3, 0)))


def finite_max(x):
    x = np.abs(np.asarray(x, np.float64))
    f = np.isfinite(x)
    return float(x[f].max()) if f.any() else 0.0


def compare_grad(got, ref, what=""):
    """Classes equal; finite elements at the trainer's tolerance (rtol 1e-5, atol 1e-6 of the
    largest finite |ref|). Returns the worst error / tolerance ratio."""
    assert got.shape == ref.shape
    cg, cr = classes(got), classes(ref)
    assert np.array_equal(cg, cr), (f"{what}: gradient classes differ at {tuple(np.argwhere(cg != cr)[0])}: "
                                    f"{got[cg != cr][0]!r} vs {ref[cg != cr][0]!r}")
    f = cr == 0
    if not f.any():
        return 0.0
    g, r = got[f].astype(np.float64), ref[f].astype(np.float64)
    tol = 1e-5 * np.abs(r) + 1e-6 * (finite_max(ref) + 1e-30)
    ratio = np.abs(g - r) / tol
    assert ratio.max() <= 1.0, f"{what}: gradient off by {ratio.max():.3g} x tolerance"
    return float(ratio.max())


def compare_ret(got, ref, what=""):
    """Per-row returns (f32 both): classes equal, finite ones within one f32 ulp of the
    reference, at most 1 + 1e-5 B of them not bit-equal. Returns the number that differ."""
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    cg, cr = classes(got), classes(ref)
    assert np.array_equal(cg, cr), f"{what}: return classes differ at rows {np.flatnonzero(cg != cr)[:5]}"
    f = cr == 0
    err = np.abs(got[f].astype(np.float64) - ref[f].astype(np.float64))
    bad = ~(err <= np.spacing(np.abs(ref[f])).astype(np.float64))
    assert not bad.any(), f"{what}: {int(bad.sum())} returns beyond one ulp: {got[f][bad][:3]} vs {ref[f][bad][:3]}"
    ndiff = int((got[f].view(np.uint32) != ref[f].view(np.uint32)).sum())
    cap = 1 + 1e-5 * got.shape[0]
    assert ndiff <= cap, f"{what}: {ndiff} returns not bit-equal (cap {cap:.2f})"
    return ndiff


def reward_close(got, ref):
    """The trainer's reward tolerance; inf compares equal to the same inf, NaN to NaN."""
    return bool(np.isclose(np.float32(got), np.float32(ref), rtol=1e-6, atol=1e-12, equal_nan=True))
