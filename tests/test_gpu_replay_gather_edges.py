"""The replay gathers (csrc/replay.h) on an MI355X where their kernels can go wrong: the
persistent F = 5 forms at every depth of their index pipelines, with one and with several
asset groups per sample, at every pairs-per-thread instantiation and both store policies
of the sequence gather; the reward fold at its chunk boundaries; the LDS and the per-float
forms at the shapes that bound them and behind misaligned pointers. Every case asserts the
kernel by its full path string first (csrc/replay_plan.h with the device's own CU count),
runs through the raw ABI with every output between sentinels, and compares every sample bit
for bit with the numpy restatement (replay_edge_inputs.py; any NaN stands for any NaN). Only
the folded reward of the n-step gather is a computed float: it is held to the f64 Horner
chain evaluated with or without fused multiply-adds in the depth cases, and to the derived
bound of the fold cases there. The conditions on the inputs are asserted on the CPU in
test_replay_edges_host.py. Needs a GPU."""
import numpy as np
import pytest
import torch

import replay_edge_inputs as E
from test_replay_plan_host import RULES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _ids(shape):
    return "x".join(map(str, shape))


def assert_path(kind, N, W, F, n, S, aligned=3, name=None):
    """The kernel the library takes for the call, by its full string: the transcribed rules of
    test_replay_plan_host.py at this device's CU count, and the instantiation the case is there for."""
    from pmenv.replay import gather_path
    got = gather_path(kind, N, W, F, n=n, S=S, aligned=aligned)
    assert got == RULES[kind](N, F, W, n, S, aligned, _cus()), got
    assert name is None or got.startswith(name + " "), (got, name)
    return got


def group(kind, N, W, F, n):
    """(G, gy) of the f5p kernel the call takes: G = max(cus / gy, 1) samples a round."""
    from pmenv.replay import gather_path
    G, gy = E.group_samples(gather_path(kind, N, W, F, n=n, S=2 ** 20))
    assert G == max(_cus() // gy, 1)
    return G, gy


def _d(e, name):
    """a table of the restatement on the device, uploaded once"""
    key = "_dev_" + name
    if key not in e.__dict__:
        e.__dict__[key] = torch.as_tensor(np.ascontiguousarray(getattr(e, name)), device=DEV)
    return e.__dict__[key]


def _bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def check_one_step(res, e, idx, what=""):
    i = torch.as_tensor(idx, device=DEV)
    assert E.same_bits(res.s, _d(e, "s")[i]), f"{what} s"
    assert E.same_bits(res.s_next, _d(e, "s_next1")[i]), f"{what} s'"
    assert E.same_bits(res.a, _d(e, "a")[i]), f"{what} a"
    assert E.same_bits(res.r, _d(e, "r")[i]), f"{what} r"


def check_nstep(res, e, idx, what="", fused_or_plain=True):
    """steps exact; s, s', a bit-equal; R bit-equal to the f64 Horner chain rounded to f32,
    its steps fused or not; discount bit-equal to the m-fold f64 product rounded to f32."""
    i = torch.as_tensor(idx, device=DEV)
    assert torch.equal(res.steps, _d(e, "m")[i]), f"{what} steps"
    assert E.same_bits(res.s, _d(e, "s")[i]), f"{what} s"
    assert E.same_bits(res.s_next, _d(e, "s_next")[i]), f"{what} s'"
    assert E.same_bits(res.a, _d(e, "a")[i]), f"{what} a"
    if not fused_or_plain:
        return
    R = _bits32(res.r.cpu().numpy())
    ok = (R == _bits32(e.R[idx])) | (R == _bits32(e.R_fused[idx]))
    assert ok.all(), f"{what} R: {np.flatnonzero(~ok)[:8]}"
    one = e.m[idx] == 1
    assert np.array_equal(R[one], _bits32(e.r[idx])[one]), f"{what} R of one step is r"
    assert np.array_equal(_bits32(res.discount.cpu().numpy()), _bits32(e.disc[idx])), f"{what} discount"


def check_seq(res, ref, idx, time_major, what=""):
    """length exact; x, a, r bit-equal, the dead elements +0.0 bits (the restatement holds
    +0.0 there and the comparison is of bits)."""
    m, live, x, a, r = ref
    i = torch.as_tensor(idx, device=DEV)
    assert torch.equal(res.length, torch.as_tensor(m, device=DEV)[i]), f"{what} length"
    got = [t.transpose(0, 1) if time_major else t for t in (res.x, res.a, res.r)]
    for g, want, name in zip(got, (x, a, r), "xar"):
        want = torch.as_tensor(want, device=DEV)[i]
        assert E.same_bits(g.contiguous(), want), f"{what} {name}"
    dead = ~torch.as_tensor(live, device=DEV)[i]
    for g, name in zip(got, "xar"):
        assert not bool(g[dead].contiguous().view(torch.int32).any()), f"{what} dead {name}"


# ---------------------------------------------------------------- 1. pipeline depth
DEPTH = [(s, k) for s in E.DEPTH_SHAPES for k in range(4)]


def _kind_n(W, k):
    return ("one_step", 1) if k == 0 else ("nstep", E.depth_n(W)[k - 1])


@pytest.mark.parametrize("label", E.S_LABELS)
@pytest.mark.parametrize("shape,k", DEPTH, ids=[f"{_ids(s)}-{'-n'.join(map(str, _kind_n(s[1], k)))}" for s, k in DEPTH])
def test_depth_sweep_of_the_persistent_gathers(shape, k, label):
    """Workgroup j % G takes sample j as its (j // G)-th: batches of 1 .. 8 samples a workgroup
    put every stage of the index chain (prologue, finish / level3 / level2 fed by the previous
    iteration, the slot rotation) in front of the restatement; (300, 4, 5) does so with two
    asset groups a sample, (514, 2, 5) with 257 groups and one workgroup column."""
    N, W, F = shape
    kind, n = _kind_n(W, k)
    G, gy = group(kind, N, W, F, n)
    S = E.s_of(label, G)
    ppt = 2 if N != 300 else 4 if n == 1 else 8
    path = assert_path(kind, N, W, F, n, S, name=f"{E.stem(kind)}_f5p_kernel<{ppt},2>")
    assert E.parse(path)[1]["grid"] == f"{min(S, G)}x{gy}"
    p, e = E.pattern(N, W, F, False, n), E.pattern_expect(N, W, F, False, n)
    for rot in E.rotations(G, p.K):
        idx = E.slots(S, G, p.K, rot)
        res = E.call(kind, p.ring, p.h0[idx], p.env[idx], n=n)
        (check_one_step if kind == "one_step" else check_nstep)(res, e, idx, f"rot {rot}")


@pytest.mark.parametrize("n,inst", E.PRODUCT_N, ids=[f"n{n}" for n, _ in E.PRODUCT_N])
def test_depth_of_the_product_shape(n, inst):
    N, W, F = E.PRODUCT
    G, gy = group("nstep", N, W, F, n)
    S = 4 * G + 1
    assert_path("nstep", N, W, F, n, S, name=f"replay_nstep_f5p_kernel{inst}")
    p, e = E.pattern(N, W, F, False, n), E.pattern_expect(N, W, F, False, n)
    idx = E.slots(S, G, p.K)
    check_nstep(E.call("nstep", p.ring, p.h0[idx], p.env[idx], n=n), e, idx)


@pytest.mark.parametrize("label", E.S_LABELS)
@pytest.mark.parametrize("shape", E.DEPTH_ENV_SHAPES, ids=_ids)
def test_depth_sweep_with_an_id_per_row_and_env(shape, label):
    """pmenv_replay_gather_nstep_env: the same chain reading ids [H, B], every column with
    boundaries and ids of its own."""
    N, W, F = shape
    n = 2 * W + 3
    G, gy = group("nstep", N, W, F, n)
    S = E.s_of(label, G)
    assert_path("nstep", N, W, F, n, S, name="replay_nstep_f5p_kernel<2,2>")
    p, e = E.pattern(N, W, F, True, n), E.pattern_expect(N, W, F, True, n)
    assert p.ring.per_env and p.ring.ids.shape == (p.ring.H, E.B)
    for rot in E.rotations(G, p.K):
        idx = E.slots(S, G, p.K, rot)
        check_nstep(E.call("nstep", p.ring, p.h0[idx], p.env[idx], n=n), e, idx, f"rot {rot}")


@pytest.mark.parametrize("per_env", [False, True], ids=["seq", "seq_env"])
def test_depth_of_the_sequence_gather(per_env):
    """5G + 1 sequences of 11 elements in chunks of 6 and 5, two asset groups: ten items a
    workgroup, every kind of sequence in front of every other."""
    (N, W, F), L = E.SEQ_DEPTH
    G, gy = group("nstep", N, W, F, L)
    S = 5 * G + 1
    path = assert_path("seq", N, W, F, L, S, name="replay_seq_f5p_kernel<8,16>")
    f = E.parse(path)[1]
    assert (f["Lc"], f["nc"]) == ("6", "2") and S * gy * 2 > 4 * int(f["grid"].split("x")[0])
    p, ref = E.pattern(N, W, F, per_env, L), E.pattern_seq(N, W, F, per_env, L)
    idx = E.slots(S, G, p.K)
    for time_major in (True, False):
        res = E.call("seq", p.ring, p.h0[idx], p.env[idx], L=L, time_major=time_major)
        check_seq(res, ref, idx, time_major, f"time_major={time_major}")


# ---------------------------------------------------------------- 2. pairs per thread
def _cycle(p, S):
    return np.arange(S) % p.K


@pytest.mark.parametrize("shape,inst", E.PPT_ONE_STEP, ids=[_ids(s) for s, _ in E.PPT_ONE_STEP])
def test_one_step_instantiations(shape, inst):
    N, W = shape
    assert_path("one_step", N, W, 5, 1, E.PPT_S, name=f"replay_gather_f5p_kernel{inst}")
    p, e = E.pattern(N, W, 5, False, 1), E.pattern_expect(N, W, 5, False, 1)
    idx = _cycle(p, E.PPT_S)
    check_one_step(E.call("one_step", p.ring, p.h0[idx], p.env[idx]), e, idx)


@pytest.mark.parametrize("shape,inst", E.PPT_NSTEP, ids=[_ids(s[:2]) + f"-n{s[2]}" for s, _ in E.PPT_NSTEP])
def test_nstep_instantiations(shape, inst):
    N, W, n = shape
    assert_path("nstep", N, W, 5, n, E.PPT_S, name=f"replay_nstep_f5p_kernel{inst}")
    p, e = E.pattern(N, W, 5, False, n), E.pattern_expect(N, W, 5, False, n)
    idx = _cycle(p, E.PPT_S)
    check_nstep(E.call("nstep", p.ring, p.h0[idx], p.env[idx], n=n), e, idx)


@pytest.mark.parametrize("shape,inst", E.PPT_SEQ, ids=[_ids(s[:2]) + f"-L{s[2]}" for s, _ in E.PPT_SEQ])
def test_sequence_instantiations(shape, inst):
    N, W, L, S = shape
    S = -(-S * _cus() // 256)                   # the chunk length follows the sequences a CU: keep their ratio
    assert_path("seq", N, W, 5, L, S, name=f"replay_seq_f5p_kernel{inst}")
    p, ref = E.pattern(N, W, 5, False, L), E.pattern_seq(N, W, 5, False, L)
    idx = _cycle(p, S)
    check_seq(E.call("seq", p.ring, p.h0[idx], p.env[idx], L=L, time_major=True), ref, idx, True)


# ---------------------------------------------------------------- 3. the sequence gather's store policy
def test_the_nt_and_the_sc1_sequence_kernels_write_the_same_windows():
    """(30, 50, 5), L = 64: 139 sequences are 254.5 MiB of windows and take <8,16>, 140 are
    256.3 MiB and take <8,2>. The first 139 of both runs, the one-step gather at every live
    element's start, and the restatement on 256 elements; the large comparisons on the device."""
    from oracle import replay_gather
    N, W, F = E.PRODUCT
    L, Sa, Sb = E.POLICY_L, E.POLICY_S16, E.POLICY_S2
    assert_path("seq", N, W, F, L, Sa, name="replay_seq_f5p_kernel<8,16>")
    assert_path("seq", N, W, F, L, Sb, name="replay_seq_f5p_kernel<8,2>")
    p = E.pattern(N, W, F, False, L)
    c, idx = p.ring, _cycle(p, Sb)
    h0, env = p.h0[idx], p.env[idx]
    sc1 = E.call("seq", c, h0[:Sa], env[:Sa], L=L)
    nt = E.call("seq", c, h0, env, L=L)
    for name in ("x", "a", "r", "length"):
        got, want = getattr(nt, name)[:Sa].float(), getattr(sc1, name).float()
        assert E.same_bits(got, want), f"<8,2> and <8,16> differ in {name}"
    del sc1
    m = p.m[idx]
    assert torch.equal(nt.length, torch.as_tensor(m, device=DEV))
    live = np.arange(L)[None, :] < m[:, None]
    jj, tt = np.nonzero(live)
    assert_path("one_step", N, W, F, 1, len(jj), name="replay_gather_f5p_kernel<8,2>")
    one = E.call("one_step", c, (h0[jj] + tt) % c.H, env[jj])
    jd, td = torch.as_tensor(jj, device=DEV), torch.as_tensor(tt, device=DEV)
    assert E.same_bits(nt.x[jd, td], one.s) and E.same_bits(nt.a[jd, td], one.a) and E.same_bits(nt.r[jd, td], one.r)
    dead = ~torch.as_tensor(live, device=DEV)
    assert not bool(nt.x[dead].view(torch.int32).any()) and not bool(nt.a[dead].view(torch.int32).any())
    assert not bool(nt.r[dead].view(torch.int32).any())
    del one
    pick = np.random.default_rng(140).choice(len(jj), 256, replace=False)
    pick[:2] = 0, len(jj) - 1
    s, a, r, _ = replay_gather(c.bars, c.days, c.actions, c.rewards, (h0[jj[pick]] + tt[pick]) % c.H, env[jj[pick]], W)
    pj, pt = jd[torch.as_tensor(pick, device=DEV)], td[torch.as_tensor(pick, device=DEV)]
    assert E.same_bits(nt.x[pj, pt], s) and E.same_bits(nt.a[pj, pt], a) and E.same_bits(nt.r[pj, pt], r)


# ---------------------------------------------------------------- 4. the fold
FOLD = [(s, name, n, g) for s, name in E.FOLD_FORMS for n in E.FOLD_N for g in E.FOLD_GAMMA]


@pytest.mark.parametrize("shape,name,n,gamma", FOLD, ids=[f"{_ids(s)}-n{n}-g{g}" for s, _, n, g in FOLD])
def test_fold_at_the_chunk_boundaries(shape, name, n, gamma):
    """nstep_fold_wave walks chunks of 64 through readlane (f5p and LDS forms), nstep_fold_serial
    a plain loop (per-float form): folds of 1, 63 .. 65, 127 .. 129 and 200 steps, gamma = 0.9
    and the ABI's upper end 1.0. |R - f32(ref)| <= ulp32(ref) + m 2^-52 sum |g^k r_k|: an f64
    Horner chain of m steps, contracted or not, and one rounding to f32."""
    N, W, F = shape
    assert_path("nstep", N, W, F, n, E.FOLD_S, name=name)
    c, e = E.fold_ring(N, W, F), E.fold_expect(N, W, F, n, gamma)
    res = E.call("nstep", c, e.h0, e.env, n=n, gamma=gamma)
    check_nstep(res, e, np.arange(E.FOLD_S), fused_or_plain=False)
    R, disc = res.r.cpu().numpy().astype(np.float64), res.discount.cpu().numpy().astype(np.float64)
    m = e.m.astype(np.float64)
    err = np.abs(R - e.R.astype(np.float32).astype(np.float64))
    bound = E.fold_bound(e.R, m, e.mag)
    print(f"fold n={n} gamma={gamma}: max |R - f32(ref)| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err / bound)
    d32 = e.disc.astype(np.float32).astype(np.float64)
    assert (np.abs(disc - d32) <= E.ulp32(e.disc)).all()
    if gamma == 1.0:
        assert (disc == 1.0).all()
        assert (np.abs(R - e.plain.astype(np.float32).astype(np.float64)) <= E.fold_bound(e.plain, m, e.mag)).all()


# ---------------------------------------------------------------- 5. generic-form boundaries
@pytest.mark.parametrize("kind,N,W,F,n,form", E.GENERIC,
                         ids=[f"{k}-{N}x{W}x{F}-n{n}" for k, N, W, F, n, _ in E.GENERIC])
def test_generic_forms_at_their_boundaries(kind, N, W, F, n, form):
    """An LDS image of exactly 64 KiB and the first shape past it, N = 256 (every thread writes
    a_out) and 257, and 45 floats a sample (the LDS kernels' scalar write-out)."""
    S = E.GENERIC_S
    path = assert_path(kind, N, W, F, n, S, name=E.stem(kind) + ("_lds_kernel" if form == "lds" else "_kernel"))
    if (N, form) == (64, "lds"):
        assert E.parse(path)[1]["lds"] == "65536"
    p = E.pattern(N, W, F, False, n)
    idx = _cycle(p, S)
    if kind == "seq":
        for time_major in (True, False):
            res = E.call("seq", p.ring, p.h0[idx], p.env[idx], L=n, time_major=time_major)
            check_seq(res, E.pattern_seq(N, W, F, False, n), idx, time_major)
        return
    res = E.call(kind, p.ring, p.h0[idx], p.env[idx], n=n)
    (check_one_step if kind == "one_step" else check_nstep)(res, E.pattern_expect(N, W, F, False, n), idx)


# ---------------------------------------------------------------- 6. alignment
ALIGN = [(s, kind, al) for s in E.ALIGN_SHAPES for kind in E.ALIGN_N for al in (2, 1, 0)]


@pytest.mark.parametrize("shape,kind,aligned", ALIGN, ids=[f"{_ids(s)}-{k}-aligned{al}" for s, k, al in ALIGN])
def test_misaligned_pointers_take_the_generic_kernels_and_give_the_same_bytes(shape, kind, aligned):
    """s / s_next / x 4 B past a 16-B boundary (aligned = 2), the series (1), both (0): the
    per-float kernels, the LDS kernels (replay_seq_kernel for sequences), the per-float kernels."""
    N, W, F = shape
    n, S = E.ALIGN_N[kind], E.ALIGN_S
    out_off, series_off = E.ALIGN_OFFS[aligned]
    assert assert_path(kind, N, W, F, n, S).startswith(E.stem(kind) + "_f5p_kernel<")
    lds = "replay_seq_kernel" if kind == "seq" else E.stem(kind) + "_lds_kernel"
    assert_path(kind, N, W, F, n, S, aligned=aligned, name=lds if aligned == 1 else E.stem(kind) + "_kernel")
    p = E.pattern(N, W, F, False, n)
    idx = _cycle(p, S)
    fast = E.call(kind, p.ring, p.h0[idx], p.env[idx], n=n, L=n)
    slow = E.call(kind, p.ring, p.h0[idx], p.env[idx], n=n, L=n, out_off=out_off, series_off=series_off)
    lead = slow.x if kind == "seq" else slow.s
    assert lead.data_ptr() % 16 == 4 * out_off
    assert E.on_device(p.ring, series_off).bars.data_ptr() % 16 == 4 * series_off
    for name, got in vars(slow).items():
        want = getattr(fast, name)
        assert E.same_bits(got.float(), want.float()) and got.dtype == want.dtype, f"{name} differs from the f5p form's"
    if kind == "seq":
        check_seq(slow, E.pattern_seq(N, W, F, False, n), idx, False)
    else:
        (check_one_step if kind == "one_step" else check_nstep)(slow, E.pattern_expect(N, W, F, False, n), idx)
