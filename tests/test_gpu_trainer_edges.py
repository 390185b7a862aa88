"""The batched reward's kernel forms (csrc/trainer.h) on the edge catalogue of
trainer_edge_inputs.py, through the raw C ABI, against the CPU oracle. Needs an MI355X.

Every call names its kernels first (pmenv_batch_reward_path against the catalogue's rules), and
runs on views into larger tensors: a, v_prev, p, grad_a, ret_out, reward_out and work sit
between sentinel-filled guards, a / p / grad_a / ret_out at base offsets of 0 - 3 floats off
16-B alignment, and work is NaN, zero or garbage before the forward. Per case:

  reward     rtol 1e-6, atol 1e-12, NaN == NaN (the trainer suite's)
  returns    NaN / +inf / -inf / finite classes equal; finite ones within one f32 ulp of the
             oracle's and at most 1 + 1e-5 B not bit-equal; work[5B + b] the expected decision
  gradient   classes equal; finite ones at rtol 1e-5, atol 1e-6 max|g|; every element written
  contained  rows the host test proved finite (all but the planted ones, under returns and
             log_returns) are finite
  guards     untouched, inputs unchanged
  bits       reward, returns and gradient bit-equal at every base offset and workspace fill
  fold       (Sharpe) work[6B + 1], work[6B + 2] against math.fsum over the chosen returns
             work[0:B) at rtol 1e-12: ~25 Chan merges of a few f64 eps each; a lost or doubled
             row is >= 1 / B ~ 1e-5

test_trainer_edges_host.py checks the catalogue itself without a GPU.
"""
import ctypes
import gc
import math

import numpy as np
import pytest
import torch

import trainer_edge_inputs as ti
from oracle import batch_reward as or_batch_reward

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KIND_ID = {"log_returns": 0, "returns": 1, "sharpe_ratio": 2}
NORM_ID = {"global_or": 0, "row_or": 1, "none": 2}
GUARD = 64                                  # elements either side: 256 B of floats
SENT32, SENT64 = 0x7FC5A5A5, 0x7FF85A5A5A5A5A5A   # quiet NaNs with a payload no kernel produces
WORST = {}                                  # assertion family -> worst observed error / tolerance


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)
    yield
    print("\nworst error / tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def _lib():
    from pmenv import _abi
    return _abi.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))


class Guarded:
    """n elements at `off` elements past a 256-B aligned base, sentinels all round."""

    def __init__(self, n, off=0, dtype=torch.float32, host=None):
        self.n, self.lo = n, GUARD + off
        self.buf = torch.empty(self.lo + n + GUARD, dtype=dtype, device=DEV)
        self.ints = self.buf.view(torch.int32 if dtype == torch.float32 else torch.int64)
        self.sent = SENT32 if dtype == torch.float32 else SENT64
        self.ints.fill_(self.sent)
        self.view = self.buf[self.lo:self.lo + n]
        assert self.view.data_ptr() % 16 == (4 * off if dtype == torch.float32 else 8 * off) % 16
        self.host = None
        if host is not None:
            self.host = np.ascontiguousarray(host).reshape(-1)
            self.view.copy_(torch.from_numpy(self.host))

    def intact(self):
        ok = bool((self.ints[:self.lo] == self.sent).all()) and bool((self.ints[self.lo + self.n:] == self.sent).all())
        if ok and self.host is not None:                      # an input: not written either
            ok = np.array_equal(self.view.cpu().numpy().view(np.uint32), self.host.view(np.uint32))
        return ok

    def all_written(self):
        return not bool((self.ints[self.lo:self.lo + self.n] == self.sent).any())


def run_raw(case, kind, norm, scale=1.0, go=1.0, offs=(0, 0, 0), fill="nan", backward=True):
    """Forward (with the per-row returns) and backward through the C ABI on guarded views.
    offs: base offsets in floats of a, p and grad_a / ret_out."""
    lib = _lib()
    B, N = case.a.shape
    a, v, p = Guarded(B * N, offs[0], host=case.a), Guarded(B, host=case.v), Guarded(B * N, offs[1], host=case.p)
    grad, ret, rew = Guarded(B * N, offs[2]), Guarded(B, offs[2]), Guarded(1)
    g = Guarded(1, host=np.array([go], np.float32))
    nw = lib.pmenv_batch_reward_workspace(B) // 8
    assert nw == 6 * B + 8 + 16 * (-(-B // 16))
    work = Guarded(nw, 0, torch.float64)
    work.view.fill_(0.0 if fill == "zero" else float("nan"))
    if fill == "garbage":
        work.view.view(torch.int32)[::3] = 0x7FFFFFF3
    s = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = lib.pmenv_batch_reward_forward(_p(a.view), _p(v.view), _p(p.view), B, N, KIND_ID[kind], NORM_ID[norm],
                                        float(scale), _p(work.view), _p(rew.view), _p(ret.view), s)
    assert rc == 0, lib.pmenv_last_error(None)
    if backward:
        rc = lib.pmenv_batch_reward_backward(_p(a.view), _p(v.view), _p(p.view), B, N, KIND_ID[kind], float(scale),
                                             _p(work.view), _p(g.view), _p(grad.view), s)
        assert rc == 0, lib.pmenv_last_error(None)
    what = f"{case.name} {kind} {norm} offs {offs} work {fill}"
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                 # a device fault: nothing more runs on this GPU
        pytest.exit(f"{what}: {e}", returncode=3)
    for name, t in (("a", a), ("v_prev", v), ("p", p), ("grad_a", grad), ("ret_out", ret), ("reward_out", rew),
                    ("grad_out", g), ("work", work)):
        assert t.intact(), f"{what}: {name}'s guards (or the input itself) were written"
    assert ret.all_written() and rew.all_written(), what
    assert not backward or grad.all_written(), f"{what}: grad_a has elements no thread stored"
    return {"reward": rew.view.cpu().numpy()[0], "ret": ret.view.cpu().numpy(), "work": work.view.cpu().numpy(),
            "grad": grad.view.cpu().numpy().reshape(B, N) if backward else None}


def check_case(case, kind, norm, scale=None, go=1.0, variants=(((0, 0, 0), "nan"),), fold=False):
    scale = case.scale if scale is None else scale
    B, N = case.a.shape
    what = f"{case.name} {kind} {norm} scale {scale} grad_out {go}"
    path = _lib().pmenv_batch_reward_path(B, N).decode()
    assert path == ti.path_rules(B, N), what
    with np.errstate(all="ignore"):
        R, oret, og = or_batch_reward(case.a, case.v, case.p, reward=kind, norm=norm, scale=scale)
        og = og * np.float32(go)
    first = None
    for offs, fill in variants:
        out = run_raw(case, kind, norm, scale, go, offs, fill)
        if first is not None:
            for k in ("reward", "ret", "grad"):
                assert np.array_equal(out[k].view(np.uint32), first[k].view(np.uint32)), \
                    f"{what}: {k} bits moved at offsets {offs}, work {fill}"
            continue
        first = out
        with np.errstate(all="ignore"):
            assert ti.reward_close(out["reward"], R), (what, path, out["reward"], R)
            if np.isfinite(R):
                r32 = float(np.float32(R))
                _note("reward", abs(float(out["reward"]) - r32) / (1e-6 * abs(r32) + 1e-12))
            _note("returns not bit-equal / cap", ti.compare_ret(out["ret"], oret, what) / (1 + 1e-5 * B))
            w = out["work"]
            flags = ti.expected_flags(case.a, norm)
            assert np.array_equal(w[5 * B:6 * B], flags.astype(np.float64)), \
                f"{what}: row flags differ at {np.flatnonzero(w[5 * B:6 * B] != flags)[:5]}"
            assert w[6 * B + 4] == NORM_ID[norm], what
            _note("gradient", ti.compare_grad(out["grad"], og, f"{what} [{path}]"))
            if kind != "sharpe_ratio":
                clean = np.setdiff1d(np.arange(B), case.planted)
                bad = clean[~np.isfinite(out["grad"][clean]).all(1)]
                assert bad.size == 0, f"{what} [{path}]: rows {bad[:8]} hold a non-finite gradient (planted: {case.planted})"
            if fold and kind == "sharpe_ratio":
                x = w[:B]
                mean = math.fsum(x) / B
                sd = math.sqrt(math.fsum((x - mean) ** 2) / (B - 1))
                for name, got, ref in (("mean", w[6 * B + 1], mean), ("std", w[6 * B + 2], sd)):
                    assert abs(got - ref) <= 1e-12 * abs(ref), f"{what} [{path}]: fold's {name} {got!r} vs {ref!r}"
                    _note("fold " + name, abs(got - ref) / (1e-12 * abs(ref)))
    return first


ALL_OFFSETS = (((0, 0, 0), "nan"), ((1, 2, 3), "zero"), ((2, 3, 1), "garbage"), ((3, 1, 2), "nan"))


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("norm", ti.NORMS)
@pytest.mark.parametrize("kind", ti.KINDS)
@pytest.mark.parametrize("N", ti.FORM_NS)
def test_gpu_batch_reward_shape_edges(N, kind, norm):
    """B either side of the small forward's limit and of every record's row count, at one N per
    kernel form; scale and grad_out take turns."""
    bwd = {5: "grad_quad_kernel<8>", 30: "grad_quad_kernel<8>", 33: "grad_quad_kernel<16>",
           64: "grad_quad_kernel<16>", 65: "grad_kernel<2>", 129: "grad_kernel<4>", 257: "grad_kernel<8>",
           513: "grad_kernel<0>"}[N]
    for i, case in enumerate(ti.shape_cases(N)):
        assert "batch_reward_" + bwd in _lib().pmenv_batch_reward_path(case.a.shape[0], N).decode()
        check_case(case, kind, norm, scale=1000.0 if i % 2 else 1.0, go=-0.5 if (i // 2) % 2 else 1.0,
                   variants=ALL_OFFSETS if N <= 64 else ALL_OFFSETS[:2])   # quad forms: 16-B loads and stores


@pytest.mark.parametrize("norm", ti.NORMS)
@pytest.mark.parametrize("kind", ti.KINDS)
@pytest.mark.parametrize("B", ti.EDGE_BS)
def test_gpu_batch_reward_n_edges(B, kind, norm):
    """N either side of every form's limit, in the small (B = 3) and the two-launch forward."""
    for i, case in enumerate(ti.n_edge_cases(B)):
        check_case(case, kind, norm, variants=ALL_OFFSETS[:1] + ALL_OFFSETS[1 + i % 3:2 + i % 3])


# ---------------------------------------------------------------- fold
@pytest.mark.parametrize("parts", ti.FOLD_PARTS)
@pytest.mark.parametrize("form", sorted(ti.FOLD_FORMS))
def test_gpu_batch_reward_fold_trip_counts(form, parts):
    """255 ... 2049 partial records: the fold's second outer trip and its k < nblk guards, with
    the marker row (return 2 among returns near 1) at each end of the batch, of the last
    record and of record 1024; the norm mode takes turns over the markers."""
    B, N = ti.fold_shape(form, parts)
    fwd, _, k = ti.parse_path(_lib().pmenv_batch_reward_path(B, N).decode())
    assert k == parts and fwd == ("batch_reward_rows_quad_kernel<8>" if form == "quad" else "batch_reward_rows_kernel<2>")
    for i, (name, row) in enumerate(ti.fold_markers(form, parts).items()):
        case = ti.fold_case(form, parts, row, ti.NORMS[i % 3])
        for kind in ti.KINDS:
            out = check_case(case, kind, case.norms[0], fold=True)
            assert abs(out["ret"][row] - 2.0) < 1e-6, (name, out["ret"][row])


# ---------------------------------------------------------------- thresholds
@pytest.mark.parametrize("B,N", ti.THRESHOLD_SHAPES)
def test_gpu_batch_reward_normalisation_threshold(B, N):
    """Batch and row sums 2^-17 and 2^-16 either side of 1 (exact in f64 in any order), and
    min = 0, -2^-24 and -0.0 at sum 1: the flags are the rule's, and the returns the chosen
    candidate's."""
    want_rows = ti.threshold_row_flags(B)
    for i, case in enumerate(ti.threshold_cases(B, N)):
        for kind in case.kinds:
            for norm in case.norms:
                out = check_case(case, kind, norm, variants=ALL_OFFSETS[i % 4:i % 4 + 1])
                if case.name.startswith("thr_rows") and norm == "row_or":
                    assert np.array_equal(out["work"][5 * B:6 * B] != 0, want_rows)


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("B,N", ti.VALUE_SHAPES)
def test_gpu_batch_reward_non_finite_values_stay_in_their_rows(B, N):
    """inf / NaN / 0 in p, v_prev and a on single rows: every element's class is the oracle's,
    and under returns / log_returns no other row loses its finite gradient - in particular not
    the row whose 16-B loads run on into the next row's inf or NaN price relative."""
    for i, case in enumerate(ti.value_cases(B, N)):
        for kind in case.kinds:
            for norm in case.norms:
                check_case(case, kind, norm, variants=ALL_OFFSETS[i % 4:i % 4 + 1])


@pytest.mark.parametrize("N", ti.FORM_NS)
def test_gpu_batch_reward_sharpe_of_one_row(N):
    case = ti.sharpe_single_row_case(N)
    for norm in case.norms:
        out = check_case(case, "sharpe_ratio", norm)
        assert np.isnan(out["reward"]) and np.isnan(out["grad"]).all()


# ---------------------------------------------------------------- wrapper
@pytest.mark.parametrize("B,N", [(64, 30), (64, 33), (65, 5), (65, 64), (33, 65), (33, 129), (17, 257), (9, 513)])
def test_gpu_batch_reward_wrapper_gives_the_raw_call_s_bits(B, N):
    """pmenv.trainer.batch_reward is the raw call: the same reward, returns and gradient bits,
    and the same gradient when backward runs twice on one forward."""
    from pmenv.trainer import batch_reward
    case = ti.shape_case(B, N)
    for kind, norm in (("log_returns", "global_or"), ("sharpe_ratio", "row_or"), ("returns", "none")):
        raw = run_raw(case, kind, norm, scale=3.0)
        a = torch.tensor(case.a, device=DEV).reshape(B, N, 1).requires_grad_(True)
        r, ret = batch_reward(a, torch.tensor(case.v, device=DEV), torch.tensor(case.p, device=DEV).reshape(B, N, 1),
                              reward=kind, scale=3.0, norm=norm, return_ret=True)
        g1, = torch.autograd.grad(r, a, retain_graph=True)
        g2, = torch.autograd.grad(r, a)
        for name, got, ref in (("reward", r.detach().reshape(1), raw["reward"].reshape(1)), ("ret", ret, raw["ret"]),
                               ("grad", g1.reshape(B, N), raw["grad"]), ("grad again", g2.reshape(B, N), raw["grad"])):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (kind, norm, name)


# ---------------------------------------------------------------- capture
@pytest.mark.parametrize("B,N", [(64, 30), (65, 33)])
def test_gpu_batch_reward_captured_update_replays_on_fresh_inputs(B, N):
    """The agents' update under hipGraph capture: forward plus backward recorded once on
    static buffers (the one-launch forward at 64 x 30, rows + fold + select at 65 x 33),
    replayed on two fresh batches, bit-equal to eager calls on the same inputs."""
    lib = _lib()
    kind, norm = "sharpe_ratio", "global_or"
    a, v, p = (torch.zeros(n, device=DEV) for n in (B * N, B, B * N))
    grad, ret, rew = torch.zeros(B * N, device=DEV), torch.zeros(B, device=DEV), torch.zeros(1, device=DEV)
    go = torch.ones(1, device=DEV)
    work = torch.full((lib.pmenv_batch_reward_workspace(B) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    # no device memory may be freed inside a capture: collect now and keep the cyclic collector off
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
            st = ctypes.c_void_p(s.cuda_stream)
            rc1 = lib.pmenv_batch_reward_forward(_p(a), _p(v), _p(p), B, N, KIND_ID[kind], NORM_ID[norm], 1.0,
                                                 _p(work), _p(rew), _p(ret), st)
            rc2 = lib.pmenv_batch_reward_backward(_p(a), _p(v), _p(p), B, N, KIND_ID[kind], 1.0, _p(work), _p(go),
                                                  _p(grad), st)
    finally:
        gc.enable()
    torch.cuda.current_stream(DEV).wait_stream(s)
    assert rc1 == 0 and rc2 == 0, lib.pmenv_last_error(None)
    for k in range(2):
        case = ti.shape_case(B + 1000 * (k + 1), N)._replace(name=f"capture_{k}")
        case = case._replace(a=case.a[:B].copy(), v=case.v[:B].copy(), p=case.p[:B].copy())
        a.copy_(torch.from_numpy(case.a.reshape(-1)))
        v.copy_(torch.from_numpy(case.v))
        p.copy_(torch.from_numpy(case.p.reshape(-1)))
        grad.fill_(float("nan"))
        work.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        got = {"reward": rew.cpu().numpy()[0], "ret": ret.cpu().numpy(), "grad": grad.cpu().numpy().reshape(B, N)}
        eager = check_case(case, kind, norm)
        for name in got:
            assert np.array_equal(got[name].view(np.uint32), eager[name].view(np.uint32)), (k, name)
