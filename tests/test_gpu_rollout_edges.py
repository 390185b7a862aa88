"""Every GAE kernel of rollout.h, the advantage moments and the trajectory metrics on the
edge-case inputs of tests/rollout_edge_inputs.py, against the CPU restatement (oracle/).

Each GAE case first asserts the kernel its shape takes (pmenv_gae_path), then the values:
  finite     every element within one f32 ulp of the oracle plus 1e-11 x its column's max,
             and at most 1 + 1e-5 T B elements not bit-equal (rollout_edge_inputs.compare_gae:
             both sides are f64 recursions rounded once);
  exact      where gamma lambda (1 - done) = 0 no composition can change a bit: adv = f32(delta);
  same bits  dones = None / all-zero dones, done bytes 2 / 128 / 255 / 1, repeated calls, the
             look-back on a workspace in any state, the tools build's forced fallback;
  guards     adv / ret inside larger tensors whose sentinel rows stay untouched;
  non-finite one poisoned element: the oracle's non-finite mask, every other env bit-equal;
  capture    a captured pmenv_gae_ex call leaves its workspace untouched and replays right.
test_rollout_edges_host.py pins the inputs' preconditions on the CPU. Needs an MI355X."""
import ctypes
import functools
import gc
import os
import warnings

import numpy as np
import pytest
import torch

import rollout_edge_inputs as ri
from oracle import gae as or_gae, moments as or_moments, trajectory_metrics as or_metrics
from test_gpu_parity import DEV, _gpu, _t  # noqa: F401  (_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS_LIB = os.path.join(ROOT, "tools", "libpmenv_ab.so")
SENTINEL = 0x7FC0DEAD                      # a NaN payload no kernel produces


def _lib():
    from pmenv import _abi
    return _abi.load()


@functools.lru_cache(maxsize=1)
def _tools():
    from pmenv import _abi
    if not os.path.exists(TOOLS_LIB):
        pytest.fail(f"{TOOLS_LIB} missing: build it with `python pm-rl_amd/build.py`")
    lib = ctypes.CDLL(TOOLS_LIB)
    for name, res, args in _abi.SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def _p(t, byte_off=0):
    return ctypes.c_void_p(t.data_ptr() + byte_off) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


@functools.lru_cache(maxsize=2)
def _batch(T, B, shift):
    """The shape's boundary batch, on the host (read-only) and on the device."""
    r, v, d = ri.gae_batch(T, B, seed=T * 7 + B, shift=shift)
    dev = (_t(r), _t(v), _t(d, torch.uint8))
    for a in (r, v, d):
        a.setflags(write=False)
    return (r, v, d), dev


@functools.lru_cache(maxsize=4)
def _oracle(T, B, shift, gamma, lam):
    r, v, d = _batch(T, B, shift)[0]
    oadv, oret = or_gae(r, v, d, gamma, lam)
    oadv.setflags(write=False)
    oret.setflags(write=False)
    return oadv, oret


def _guarded(T, B):
    """[T, B] f32 inside a [T + 2, B] tensor whose first and last rows are sentinels."""
    buf = torch.full((T + 2, B), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[1:T + 1].view(torch.float32)


def _guards_ok(buf):
    return bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())


def _raw(through, r, v, d, T, B, gamma, lam, lib=None, work="own", nbytes=None, work_off=0):
    """One call through the raw ABI into guarded outputs: through = "gae" is pmenv_gae_ex (work =
    "own": scratch of pmenv_gae_workspace bytes; else the tensor given, or None), "direct" is
    pmenv_gae. Returns (adv, ret) device tensors; the guards are asserted."""
    lib = lib or _lib()
    abuf, adv = _guarded(T, B)
    rbuf, ret = _guarded(T, B)
    if through == "direct":
        rc = lib.pmenv_gae(_p(r), _p(v), _p(d), _p(adv), _p(ret), T, B, gamma, lam, _stream())
    else:
        if isinstance(work, str):
            nbytes = lib.pmenv_gae_workspace(T, B)
            work = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV) if nbytes else None
        rc = lib.pmenv_gae_ex(_p(r), _p(v), _p(d), _p(adv), _p(ret), T, B, gamma, lam, _p(work, work_off),
                              nbytes or 0, _stream())
    assert rc == 0, lib.pmenv_last_error(None)
    torch.cuda.synchronize()
    assert _guards_ok(abuf) and _guards_ok(rbuf), "a sentinel row around adv / ret was written"
    return adv, ret


def _run(through, r, v, d, T, B, gamma, lam):
    """As the case table says: rollout.gae, or pmenv_gae through the raw ABI."""
    from pmenv import rollout
    if through == "gae":
        return rollout.gae(r, v, d, gamma, lam)
    return _raw("direct", r, v, d, T, B, gamma, lam)


def _path(through, T, B):
    from pmenv import rollout
    return rollout.gae_path(T, B, workspace=through == "gae")


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_values(adv, ret, T, B, shift, gamma, lam, what):
    (r, v, d), _ = _batch(T, B, shift)
    oadv, oret = _oracle(T, B, shift, gamma, lam)
    adv, ret = adv.cpu().numpy(), ret.cpu().numpy()
    ri.compare_gae(adv, oadv, f"{what} adv")
    ri.compare_gae(ret, oret, f"{what} ret")
    # exact: delta + 0 * x = delta
    eadv, eret = ri.delta_exact(r, v, d, gamma)
    if gamma * lam == 0.0:
        cols = slice(None)
    else:
        cols = np.flatnonzero((np.arange(B) + shift) % ri.K == ri.CLASS["every"])
    assert np.array_equal(adv[:, cols].view(np.uint32), eadv[:, cols].view(np.uint32)), f"{what}: adv != f32(delta)"
    assert np.array_equal(ret[:, cols].view(np.uint32), eret[:, cols].view(np.uint32)), f"{what}: ret != f32(delta + v)"


# ---------------------------------------------------------------------------- finite
@pytest.mark.parametrize("gamma,lam", ri.GAMMA_LAMBDA)
@pytest.mark.parametrize("kernel,through,T,B,shift", ri.GAE_CASES)
def test_gpu_gae_edges_match_oracle(kernel, through, T, B, shift, gamma, lam):
    assert _path(through, T, B) == kernel
    _, (r, v, d) = _batch(T, B, shift)
    adv, ret = _run(through, r, v, d, T, B, gamma, lam)
    _check_values(adv, ret, T, B, shift, gamma, lam, f"{kernel} ({T}, {B})")


# ------------------------------------------------------------------- same bits, guards
def _same_bits_body(raw, T, B, shift, what):
    """raw(r, v, d) -> (adv, ret) through the raw ABI into guarded outputs at (0.99, 0.95)."""
    (_, _, dh), (r, v, d) = _batch(T, B, shift)
    adv, ret = raw(r, v, d)
    _check_values(adv, ret, T, B, shift, 0.99, 0.95, f"{what} ({T}, {B}) raw")
    for i in range(2):
        a2, r2 = raw(r, v, d)
        assert _same(a2, adv) and _same(r2, ret), f"call {i + 2} differs from call 1"
    a3, r3 = raw(r, v, _t(ri.stamp_done_bytes(dh), torch.uint8))
    assert _same(a3, adv) and _same(r3, ret), "done bytes 2 / 128 / 255 differ from 1"
    an, rn = raw(r, v, None)
    az, rz = raw(r, v, torch.zeros_like(d))
    assert _same(an, az) and _same(rn, rz), "dones = NULL differs from all-zero dones"
    return az


@pytest.mark.parametrize("kernel,through,T,B,shift", ri.GAE_CASES)
def test_gpu_gae_edges_same_bits_and_guards(kernel, through, T, B, shift):
    """Through the raw ABI into guarded outputs (ragged B: lanes past B must store nothing):
    the oracle's values; three calls, the same bits; done bytes 2 / 128 / 255 as 1; dones = NULL
    as all-zero dones (the zero-record descriptor reads 0)."""
    assert _path(through, T, B) == kernel
    az = _same_bits_body(lambda r, v, d: _raw(through, r, v, d, T, B, 0.99, 0.95), T, B, shift, kernel)
    a0, _ = _run(through, _batch(T, B, shift)[1][0], _batch(T, B, shift)[1][1], None, T, B, 0.99, 0.95)
    assert _same(a0, az)


LB_SHAPES = [(513, 65), (700, 67), (1025, 900)]


@pytest.mark.parametrize("T,B", LB_SHAPES)
def test_gpu_gae_lookback_workspace_in_any_state(T, B):
    """The look-back through the raw ABI on a workspace of exactly pmenv_gae_workspace bytes:
    fresh, pre-filled with NaN and garbage words, and still holding the previous call's content
    for a different shape — the same bits (a flag counts only with this call's epoch)."""
    lib = _lib()
    assert _path("gae", T, B).startswith("gae_lookback_kernel")
    _, (r, v, d) = _batch(T, B, 0)
    nbytes = lib.pmenv_gae_workspace(T, B)
    fresh = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
    adv, ret = _raw("gae", r, v, d, T, B, 0.99, 0.95, work=fresh, nbytes=nbytes)
    _check_values(adv, ret, T, B, 0, 0.99, 0.95, f"look-back ({T}, {B})")
    g = torch.Generator(device=DEV).manual_seed(T)
    junk = torch.randint(-2 ** 62, 2 ** 62, (nbytes // 8,), generator=g, device=DEV, dtype=torch.int64)
    junk[::3] = torch.tensor(float("nan"), dtype=torch.float64).view(torch.int64).item()
    a2, r2 = _raw("gae", r, v, d, T, B, 0.99, 0.95, work=junk.view(torch.float64), nbytes=nbytes)
    assert _same(a2, adv) and _same(r2, ret), "garbage workspace"
    # the previous call's content for a different shape: other chunk count, other env blocks
    T2, B2 = T + 190, B // 3
    n2 = lib.pmenv_gae_workspace(T2, B2)
    assert 0 < n2 <= nbytes and _path("gae", T2, B2).startswith("gae_lookback_kernel")
    (_, _, _), (rb, vb, db) = _batch(T2, B2, 0)
    work = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
    ab, _ = _raw("gae", rb, vb, db, T2, B2, 0.99, 0.95, work=work, nbytes=nbytes)
    ri.compare_gae(ab.cpu().numpy(), or_gae(*_batch(T2, B2, 0)[0], 0.99, 0.95)[0], "the other shape")
    a3, r3 = _raw("gae", r, v, d, T, B, 0.99, 0.95, work=work, nbytes=nbytes)
    assert _same(a3, adv) and _same(r3, ret), "workspace left by another shape"
    a4, r4 = _raw("gae", r, v, d, T, B, 0.99, 0.95, work=work, nbytes=nbytes)
    assert _same(a4, adv) and _same(r4, ret), "workspace left by the same shape"


@pytest.mark.parametrize("T,B", [(513, 65), (1025, 900)])
def test_gpu_gae_ex_fallbacks_take_the_gae_path(T, B):
    """work = NULL, work_bytes 8 short and work 4 bytes off alignment: as pmenv_gae (pmenv_gae_path
    says so), the oracle's values, and the workspace left untouched."""
    lib = _lib()
    need = lib.pmenv_gae_workspace(T, B)
    _, (r, v, d) = _batch(T, B, 0)
    direct, _ = _raw("direct", r, v, d, T, B, 0.99, 0.95)
    pat = 0x5A5A5A5A5A5A5A5A
    for what, null, nbytes, off in [("NULL", True, need, 0), ("short", False, need - 8, 0),
                                    ("misaligned", False, need, 4)]:
        assert lib.pmenv_gae_path(T, B, 0 if null else nbytes, int(not null and off % 8 == 0)).decode() == ri.TILE16
        work = torch.full((need // 8 + 1,), pat, dtype=torch.int64, device=DEV)
        adv, ret = _raw("gae", r, v, d, T, B, 0.99, 0.95, work=None if null else work.view(torch.float64),
                        nbytes=nbytes, work_off=off)
        _check_values(adv, ret, T, B, 0, 0.99, 0.95, f"{what} ({T}, {B})")
        assert _same(adv, direct), what
        assert bool((work == pat).all()), f"{what}: the workspace was written"


# ------------------------------------------------------------------------- tools build
class _knob:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _tools_run(knob, through):
    """A call of the tools build with PMENV_GAE=knob set around it (read at call time)."""
    def run(r, v, d, T, B, gamma=0.99, lam=0.95):
        with _knob(PMENV_GAE=knob):
            return _raw(through, r, v, d, T, B, gamma, lam, lib=_tools())
    return run


@pytest.mark.parametrize("T,B,shift", ri.LOOP_CASES)
def test_gpu_gae_loop_kernel_carries(T, B, shift):
    """gae_kernel (the per-env loop) with T > 1, so its carry is used: the product reaches it
    only from 2 GiB rollouts, the tools build's PMENV_GAE=loop launches the same kernel of
    rollout.h at any shape. The finite and exact legs at every (gamma, lambda), then the same-bits
    and guard legs."""
    assert _path("gae", T, B) != ri.LOOP          # the product's rule; the knob overrides it
    run = _tools_run("loop", "direct")
    _, (r, v, d) = _batch(T, B, shift)
    for gamma, lam in ri.GAMMA_LAMBDA:
        adv, ret = run(r, v, d, T, B, gamma, lam)
        _check_values(adv, ret, T, B, shift, gamma, lam, f"gae_kernel ({T}, {B})")
    _same_bits_body(lambda r, v, d: run(r, v, d, T, B), T, B, shift, "gae_kernel")


@pytest.mark.parametrize("T,B,shift", ri.FALLBACK_CASES)
def test_gpu_gae_lookback_forced_fallback_gives_the_product_bits(T, B, shift):
    """The look-back's forward-progress fallback (a wave that finds a flag missing computes that
    chunk's map itself): the tools build's SPIN = 0 form of the same kernel, bit-equal to the
    product."""
    assert _path("gae", T, B).startswith("gae_lookback_kernel")
    run = _tools_run("lbfb", "gae")
    _, (r, v, d) = _batch(T, B, shift)
    adv, ret = _raw("gae", r, v, d, T, B, 0.99, 0.95)
    _check_values(adv, ret, T, B, shift, 0.99, 0.95, f"look-back ({T}, {B})")
    for dd in (d, None):
        pa, pr = _raw("gae", r, v, dd, T, B, 0.99, 1.0)
        fa, fr = run(r, v, dd, T, B, 0.99, 1.0)
        assert _same(fa, pa) and _same(fr, pr)


# -------------------------------------------------------------------------- non-finite
def _poison_points(kernel, T, B):
    if kernel == ri.SCAN:
        p0, p1 = ri.scan_pieces(T)[len(ri.scan_pieces(T)) // 2]
    else:
        parts = ri.pieces(T, *ri.GEOMETRY[kernel])
        p0, p1 = parts[len(parts) // 2]
    b63, b64 = min(63, B - 1), min(64, B - 1)
    return [("r", 0, 0, "nan"), ("v", T - 1, b63, "+inf"), ("r", p1, b64, "-inf"), ("v", p0, B - 1, "nan"),
            ("r", T - 1, b64, "+inf"), ("v", p1, 0, "-inf"), ("v", T, b63, "nan"), ("v", T, B - 1, "+inf")]


def _nonfinite_body(run, points, T, B, shift, twin=None):
    """run(r, v, d) -> (adv, ret) at (0.99, 0.95). One poisoned element per run: the non-finite
    mask of the env's adv and ret is the oracle's, and every other env's column is bit-equal to
    the unpoisoned run. twin: a second runner whose poisoned output must have the same bits."""
    (rh, vh, dh), (r, v, d) = _batch(T, B, shift)
    adv0, ret0 = run(r, v, d)
    other = torch.ones(B, dtype=torch.bool, device=DEV)
    for what, t0, b0, value in points:
        src = r if what == "r" else v
        keep = src[t0, b0].item()
        src[t0, b0] = ri.POISON_VALUES[value]
        try:
            adv, ret = run(r, v, d)
            tw = twin(r, v, d) if twin else None
            torch.cuda.synchronize()
        finally:
            src[t0, b0] = keep
        tag = f"{what}[{t0}, {b0}] = {value}"
        if tw is not None:
            assert _same(tw[0], adv) and _same(tw[1], ret), f"{tag}: differs from the product's poisoned output"
        other[:] = True
        other[b0] = False
        assert _same(adv[:, other], adv0[:, other]) and _same(ret[:, other], ret0[:, other]), f"{tag}: another env moved"
        r1, v1 = ri.poison(rh[:, b0:b0 + 1], vh[:, b0:b0 + 1], what, t0, 0, value)
        with np.errstate(all="ignore"):
            oadv, oret = or_gae(r1, v1, np.ascontiguousarray(dh[:, b0:b0 + 1]), 0.99, 0.95)
        for got, exp, name in ((adv[:, b0].cpu().numpy(), oadv[:, 0], "adv"), (ret[:, b0].cpu().numpy(), oret[:, 0], "ret")):
            for f in (np.isnan, np.isposinf, np.isneginf):
                assert np.array_equal(f(got), f(exp)), f"{tag}: {name} {f.__name__} mask"
            # the column's maximum is non-finite here, so the finite elements (the days after the
            # poison) are held to one ulp plus 1e-11 x their own maximum; no count of unequal bits
            fin = np.isfinite(exp)
            assert np.all(np.abs(got[fin].astype(np.float64) - exp[fin]) <=
                          np.spacing(np.abs(exp[fin])) + 1e-11 * np.abs(exp[fin]).max(initial=0.0)), f"{tag}: {name}"
        assert not np.isfinite(oadv).all(), f"{tag}: the poison reached nothing"


@pytest.mark.parametrize("kernel,through,T,B,shift", ri.POISON_CASES)
def test_gpu_gae_nonfinite_stays_in_its_env(kernel, through, T, B, shift):
    """One poisoned element per run (day 0, day T - 1, a piece's last and first day, v's bootstrap
    row T; envs 0, 63, 64, B - 1): the non-finite mask of the env's adv and ret is the oracle's
    (0 * NaN is NaN: a done does not stop it), its finite elements are within one ulp of the
    oracle's, and every other env's column is bit-equal to the unpoisoned run."""
    assert _path(through, T, B) == kernel
    _nonfinite_body(lambda r, v, d: _run(through, r, v, d, T, B, 0.99, 0.95), _poison_points(kernel, T, B),
                    T, B, shift)


@pytest.mark.parametrize("T,B,shift", ri.LOOP_CASES)
def test_gpu_gae_loop_kernel_nonfinite_stays_in_its_env(T, B, shift):
    """The non-finite leg on gae_kernel (tools build, PMENV_GAE=loop): days 0, T / 2, T - 1 and the
    bootstrap row T at envs 0, 63, 64, B - 1."""
    assert _path("gae", T, B) != ri.LOOP
    run = _tools_run("loop", "direct")
    b63, b64 = min(63, B - 1), min(64, B - 1)
    points = [("r", 0, 0, "nan"), ("v", T // 2, b63, "+inf"), ("r", T - 1, b64, "-inf"), ("v", T, B - 1, "nan"),
              ("v", T // 2, 0, "-inf"), ("r", T // 2, B - 1, "+inf"), ("v", T - 1, b64, "nan"), ("v", T, b63, "+inf")]
    _nonfinite_body(lambda r, v, d: run(r, v, d, T, B), points, T, B, shift)


@pytest.mark.parametrize("T,B,shift", ri.FALLBACK_CASES)
def test_gpu_gae_lookback_fallback_nonfinite_stays_in_its_env(T, B, shift):
    """The non-finite leg on the look-back's forced fallback (tools build, PMENV_GAE=lbfb); every
    poisoned output also bit-equal to the product's on the same poisoned input."""
    kernel = _path("gae", T, B)
    assert kernel.startswith("gae_lookback_kernel")
    run = _tools_run("lbfb", "gae")
    _nonfinite_body(lambda r, v, d: run(r, v, d, T, B), _poison_points(kernel, T, B), T, B, shift,
                    twin=lambda r, v, d: _raw("gae", r, v, d, T, B, 0.99, 0.95))


# ----------------------------------------------------------------------------- capture
@pytest.mark.parametrize("T,B", [(513, 65), (1025, 900), (300, 130)])
def test_gpu_gae_ex_under_graph_capture(T, B):
    """One pmenv_gae_ex call captured on static buffers and replayed three times with fresh
    inputs: the look-back's epoch is a host-chosen kernel argument, which a replay would reuse
    on flags that already carry it, so a captured call takes the pmenv_gae path — the workspace,
    pre-filled with a sentinel, is byte-identical after the replays, and every replay matches the
    oracle."""
    lib = _lib()
    nbytes = lib.pmenv_gae_workspace(T, B)
    pat = 0x5A5A5A5A5A5A5A5A
    work = torch.full((max(nbytes // 8, 1),), pat, dtype=torch.int64, device=DEV)
    r = torch.zeros(T, B, device=DEV)
    v = torch.zeros(T + 1, B, device=DEV)
    d = torch.zeros(T, B, dtype=torch.uint8, device=DEV)
    abuf, adv = _guarded(T, B)
    rbuf, ret = _guarded(T, B)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    # Freeing device memory or destroying a graph during a global-mode capture invalidates the
    # capture, and the runtime error surfaces in a destructor (an abort). Python's cyclic collector
    # can do exactly that at any allocation inside the region if a dead cycle holds tensors or a
    # CUDAGraph; torch.cuda.graph collects before a capture only when force_cudagraph_gc is set.
    # So: collect now, and keep the collector off inside the region.
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
            rc = lib.pmenv_gae_ex(_p(r), _p(v), _p(d), _p(adv), _p(ret), T, B, 0.99, 0.95,
                                  _p(work) if nbytes else None, nbytes, ctypes.c_void_p(s.cuda_stream))
    finally:
        gc.enable()
    torch.cuda.current_stream(DEV).wait_stream(s)
    assert rc == 0, lib.pmenv_last_error(None)
    outs = []
    for k in range(3):
        rh, vh, dh = ri.gae_batch(T, B, seed=100 + k, shift=k)
        r.copy_(_t(rh))
        v.copy_(_t(vh))
        d.copy_(_t(dh, torch.uint8))
        g.replay()
        torch.cuda.synchronize()
        outs.append((adv.cpu().numpy(), ret.cpu().numpy(), or_gae(rh, vh, dh, 0.99, 0.95)))
    # the deterministic check first (a stale read of the previous replay's maps is a race)
    assert bool((work == pat).all()), "a captured pmenv_gae_ex wrote its workspace: the look-back ran under capture"
    assert _guards_ok(abuf) and _guards_ok(rbuf)
    for k, (a, rr, (oadv, oret)) in enumerate(outs):
        ri.compare_gae(a, oadv, f"replay {k} adv")
        ri.compare_gae(rr, oret, f"replay {k} ret")
    # eager calls on the same workspace afterwards take the look-back again
    if nbytes:
        a2, _ = _raw("gae", r, v, d, T, B, 0.99, 0.95, work=work.view(torch.float64), nbytes=nbytes)
        ri.compare_gae(a2.cpu().numpy(), oadv, "eager after capture")
        assert not bool((work == pat).all())


# ----------------------------------------------------------------------------- moments
@pytest.mark.parametrize("kind", ["normal", "integer"])
@pytest.mark.parametrize("n,off", [(4_200_003, 0), (4_200_003, 1)])
def test_gpu_moments_block_cap_and_exact_sums(n, off, kind):
    """n = 4,200,003 engages the 1,024-block cap and the four-deep grid stride. Integer values
    in -8 .. 8: sum and sum of squares are exact in f64 in any order, so the result must equal
    the oracle's bit for bit."""
    from pmenv import rollout
    rng = np.random.default_rng(n + off)
    if kind == "integer":
        x = rng.integers(-8, 9, n + off).astype(np.float32)
    else:
        x = rng.standard_normal(n + off).astype(np.float32)
    m = rollout.moments(_t(x)[off:]).cpu().numpy()
    om = or_moments(np.ascontiguousarray(x[off:]))
    assert m[0] == om[0] == n
    if kind == "integer":
        assert np.array_equal(m.view(np.uint64), om.view(np.uint64)), (m, om)
    else:
        np.testing.assert_allclose(m[1:], om[1:], rtol=1e-9, atol=1e-9)


# ----------------------------------------------------------------------------- metrics
KEYS = ("sharpe", "sortino", "max_drawdown", "average_turnover", "final_value")


def _gpu_metrics(ret, val, w, rf, periods):
    from pmenv.replay import trajectory_metrics
    got = trajectory_metrics(_t(ret, torch.float64), _t(val, torch.float64), _t(w), rf, periods)
    return torch.stack([got[k] for k in KEYS], 1).cpu().numpy()


@pytest.mark.parametrize("rf,periods", ri.METRIC_RATES)
@pytest.mark.parametrize("T,B,N", ri.METRIC_SHAPES)
def test_gpu_metrics_edges_match_restatement(T, B, N, rf, periods):
    """trajectory_metrics on the degenerate classes (constant, zero, all-positive, one big first
    day, monotone values, peaks on the wave segments' first days, alternating weights), T = 1 .. 7
    (every remainder of the 4-unrolled loops, empty wave segments), N across 256, both rf
    branches: the restatement's values at rtol 1e-6 / atol 1e-9 with an identical inf / NaN
    pattern (test_rollout_edges_host.py pins the restatement's own pattern on the zero-deviation
    classes at every rate: sign(mean) x inf)."""
    ret, val, w = ri.metrics_batch(T, B, N, seed=T * 31 + N)
    got = _gpu_metrics(ret, val, w, rf, periods)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        exp = or_metrics(ret, val, w, rf=rf, periods=periods)
    for i, k in enumerate(KEYS):
        for f in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(f(got[:, i]), f(exp[:, i])), f"{k}: {f.__name__} pattern"
        fin = np.isfinite(exp[:, i])
        np.testing.assert_allclose(got[fin, i], exp[fin, i], rtol=1e-6, atol=1e-9, err_msg=k)
    for b in range(B):                             # closed-form turnover
        if b % ri.KM == ri.MCLASS["alt_weights"]:
            np.testing.assert_allclose(got[b, 3], ri.alt_turnover(w, b), rtol=1e-12)
    assert np.array_equal(got[:, 4], val[-1])


@pytest.mark.parametrize("T,B,N", [(3, 65, 30), (7, 130, 257), (64, 129, 30)])
def test_gpu_metrics_nan_stays_in_its_env(T, B, N):
    """A NaN in one env's returns, values or weights leaves every other env's five outputs
    bit-equal (lanes are envs; lanes past B read env B - 1 and store nothing). The poisoned env's
    own outputs are left unpinned: the reference's module (quantstats) is absent, and pandas
    skips NaN where the numpy restatement propagates it."""
    ret, val, w = ri.metrics_batch(T, B, N, seed=T * 31 + N)
    base = _gpu_metrics(ret, val, w, 0.04, 252.0)
    for what, t0, b0 in [("ret", 0, 0), ("ret", T - 1, B - 1), ("val", T, 63), ("val", (T + 1) // 4, 64),
                         ("w", T // 2, B - 1), ("w", 0, 63)]:
        r2, v2, w2 = ret.copy(), val.copy(), w.copy()
        if what == "w":
            w2[t0, b0, N - 1] = np.nan
        else:
            (r2 if what == "ret" else v2)[t0, b0] = np.nan
        got = _gpu_metrics(r2, v2, w2, 0.04, 252.0)
        keep = np.arange(B) != b0
        assert np.array_equal(got[keep].view(np.uint64), base[keep].view(np.uint64)), (what, t0, b0)
