"""pmenv_rollout_gather and pmenv_rollout_gather_env on an MI355X where their four kernels
(csrc/replay.h) can go wrong: every form the plan chooses (csrc/replay_plan.h) at the
shapes that bound it, F != 5, both rings around the storage-order wrap, windows that leave
the series at either end, misaligned outputs and series, and both store policies of the
tile form. Every test asserts the kernel by name first and then compares bit for bit with
the numpy data model (rollout_window_ref.py, itself checked in
test_rollout_window_model_host.py); any NaN stands for any NaN, nothing has a tolerance.
Needs a GPU."""
import functools
import types

import numpy as np
import pytest
import torch

from rollout_window_ref import lockstep_ref, window_ref
from test_gpu_rollout_episodes import _drive, _roles, gather_env, gather_lockstep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RINGS = ["storage", "chrono"]
B = 5                                    # envs of the raw-ABI tests: one per start day below
GUARD = 64                               # sentinel floats on either side of an output (256 B: keeps 16-B alignment)
SENTINEL = -7.5                          # no window holds it: bars > 0, weights in {0, 1} or [0.5, 1.5)

# (N, W, F), the form the plan's rule gives — tile iff F = 5, N*W % 4 == 0, N*W*20 <= 65,536 and
# both pointers 16-B aligned — and the edge the shape is there for
SWEEP = [
    (1, 4, 5, "tile"),       # one asset: make_fastdiv(1), nd = 4
    (4, 1, 5, "tile"),       # W = 1 (against the data model alone)
    (8, 32, 5, "tile"),      # nd = 256: one (day, asset) pair per thread
    (32, 32, 5, "tile"),     # nd = 1,024: exactly one staging round
    (257, 4, 5, "tile"),     # nd = 1,028: four pairs into a second round; N > 256
    (63, 52, 5, "tile"),     # nd = 3,276: the largest tile, 65,520 B of LDS
    (41, 80, 5, "rows"),     # nd = 3,280: 16-B granular but 65,600 B, the first past the limit; 400-float rows
    (257, 3, 5, "rows"),     # N > 256
    (3, 13, 5, "rows"),      # 65-float rows: one lane into the second load
    (3, 8, 8, "rows"),       # 64-float rows, F = 8
    (3, 64, 8, "rows"),      # 512-float rows: the last unrolled size
    (3, 103, 5, "rows"),     # 515 floats: the first looped size
    (2, 65, 8, "rows"),      # 520 floats, looped, F = 8
    (1, 301, 5, "rows"),     # 1,505-float rows, one asset
    (5, 9, 2, "rows"),       # F = 2: one market channel
    (6, 10, 3, "rows"),      # F = 3
]
IDS = ["x".join(map(str, s[:3])) for s in SWEEP]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


# ---------------------------------------------------------------- inputs, built once per shape
def _ts(W):
    T = 2 * W + 3
    return sorted({min(max(t, 0), T) for t in (0, 1, W - 2, W - 1, W, W + 1, 2 * W - 1, 2 * W, T)})


def _f32(x):
    return torch.as_tensor(np.array(x, np.float32), device=DEV)             # a copy: x may be frozen


def _i32(x):
    return torch.as_tensor(np.array(x, np.int32), device=DEV)


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _case(N, W, F):
    """The sweep's buffers for a shape: T_rec = 2W + 3 recorded steps of B = 5 envs over a series of
    W + T_rec + 6 days, the lockstep start days (one env per place a window can lie) and the
    edge samples, every env at each step."""
    c = types.SimpleNamespace(N=N, W=W, F=F, T=2 * W + 3)
    c.Ts = W + c.T + 6
    rng = np.random.default_rng(1000 * N + 10 * W + F)
    c.bars = _frozen((100 * np.exp(0.01 * rng.standard_normal((c.Ts, N, F - 1)).cumsum(0))).astype(np.float32))
    c.weights = _frozen((rng.random((c.T, B, N)) + 0.5).astype(np.float32))
    c.start = _frozen(np.array([-W - 1,          # wholly before day 0 at t = 0
                                -2,              # partly before
                                c.Ts - W - 1,    # runs past the end from t = 2
                                c.Ts + 1,        # wholly past
                                3]))             # wholly inside for every t: 3 + T_rec + W - 1 < Ts
    assert c.start[4] >= 0 and c.start[4] + c.T + W <= c.Ts
    ts = _ts(W)
    c.t = _frozen(np.repeat(ts, B))
    c.e = _frozen(np.tile(np.arange(B), len(ts)))
    c.S = c.t.size
    c.series = types.SimpleNamespace(bars=_f32(c.bars))
    c.start_d, c.weights_d, c.t_d, c.e_d = _i32(c.start), _f32(c.weights), _i32(c.t), _i32(c.e)
    assert c.series.bars.data_ptr() % 16 == 0
    tcol = np.arange(c.T + 1)[:, None]
    c.first_lock = _frozen(c.start[None, :] + tcol)
    c.updates_lock = _frozen(np.repeat(tcol, B, 1))
    return c


@functools.lru_cache(maxsize=None)
def _books(N, W, F, carry):
    """Per-env bookkeeping of its own, as test_gpu_rollout_episodes.py's section 4 draws it: first
    inside the series and off both ends, updates inside the contract (<= t + carry) and, env 2,
    beyond it; weights [carry + T_rec, B, N]."""
    c = _case(N, W, F)
    rng = np.random.default_rng(7 * N + 3 * W + F + carry)
    T, Ts = c.T, c.Ts
    k = types.SimpleNamespace(carry=carry)
    first = rng.integers(0, Ts - W + 1, (T + 1, B))
    first[:, 0] = Ts - W + 1 + rng.integers(0, W + 3, T + 1)          # env 0: runs past the end, or lies past it
    first[:, 1] = -rng.integers(1, W + 3, T + 1)                      # env 1: begins before day 0, or lies before it
    first[T, 3] = Ts                                                # wholly outside
    tcol = np.arange(T + 1)[:, None]
    updates = rng.integers(0, tcol + carry + 1, (T + 1, B))          # in contract: <= t + carry
    updates[:, 2] = tcol[:, 0] + carry + 1 + rng.integers(0, 2 * W, T + 1)   # env 2: beyond it (reads 0, never memory)
    k.first, k.updates = _frozen(first), _frozen(updates)
    k.weights = _frozen((rng.random((carry + T, B, N)) + 0.5).astype(np.float32))
    k.first_d, k.updates_d, k.weights_d = _i32(first), _i32(updates), _f32(k.weights)
    return k


@functools.lru_cache(maxsize=None)
def _lockstep_want(N, W, F, ring):
    c = _case(N, W, F)
    return _frozen(np.stack([lockstep_ref(c.bars, c.start, c.weights, W, ring, t, b) for t, b in zip(c.t, c.e)]))


@functools.lru_cache(maxsize=None)
def _env_want(N, W, F, ring, carry):
    c, k = _case(N, W, F), _books(N, W, F, carry)
    return _frozen(np.stack([window_ref(c.bars, k.first, k.updates, k.weights, carry, W, ring, t, b)
                             for t, b in zip(c.t, c.e)]))


# ---------------------------------------------------------------- names, guards, bits
def _expect(N, W, F, S, form, policy=16, env=False):
    stem = "rollout_gather_env_" if env else "rollout_gather_"
    if form == "tile":
        return f"{stem}tile_kernel<{policy}> R=0 grid={S}x1 lds={N * W * 20}"
    return f"{stem}rows_kernel R=0 grid={(S * N + 3) // 4}x1 lds=0"


def _assert_names(N, W, F, S, form, aligned=3, policy=16):
    """Both entry points' kernels for the shape, as the library names its plan."""
    from pmenv import _abi
    from pmenv.replay import gather_path
    assert gather_path("rollout", N, W, F, S=S, aligned=aligned) == _expect(N, W, F, S, form, policy)
    env_path = _abi.load().pmenv_rollout_gather_env_path(N, F, W, S, aligned).decode()
    assert env_path == _expect(N, W, F, S, form, policy, env=True)


def _guarded(n, off=0):
    """n output floats `off` floats past a 16-B boundary, between two runs of sentinels."""
    raw = torch.full((n + 2 * GUARD + 4,), SENTINEL, device=DEV)
    assert raw.data_ptr() % 16 == 0
    view = raw[GUARD + off:GUARD + off + n]
    assert view.data_ptr() % 16 == 4 * off
    return raw, view


def _assert_guards(raw, n, off=0):
    lo, hi = raw[:GUARD + off], raw[GUARD + off + n:]
    assert hi.numel() >= GUARD
    assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), "a store outside the output"


def _canon(a):
    """float32 numpy -> int32 bits with one NaN for all"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), a).view(np.int32)


def _canon_d(x):
    x = x.contiguous()
    return torch.where(torch.isnan(x), torch.full_like(x, float("nan")), x).view(torch.int32)


def _assert_bits(got, want, what):
    got, want = _canon(got), _canon(want)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)
        j, n, p, f = at[0]
        raise AssertionError(f"{what}: {len(at)} floats differ, the first at (sample, asset, day, channel) = "
                             f"({j}, {n}, {p}, {f}): {got.view(np.float32)[j, n, p, f]!r} for "
                             f"{want.view(np.float32)[j, n, p, f]!r}")


def _assert_nan_outside(got, d0, Ts, F):
    """market channels NaN exactly at the days outside the series, the weight channel finite"""
    W = got.shape[2]
    day = np.asarray(d0)[:, None] + np.arange(W)[None, :]
    outside = (day < 0) | (day >= Ts)
    nan = np.isnan(got[..., :F - 1])
    assert np.array_equal(nan.all(axis=(1, 3)), outside) and np.array_equal(nan.any(axis=(1, 3)), outside)
    assert np.isfinite(got[..., F - 1]).all()
    return outside


def _run(fn, shape, off=0):
    """fn(out=view) into a guarded output; the host copy, the device view, guards checked"""
    n = int(np.prod(shape))
    raw, view = _guarded(n, off)
    fn(out=view)
    _assert_guards(raw, n, off)
    assert not bool((view == SENTINEL).any()), "a float was not written"
    return view.view(*shape)


# ---------------------------------------------------------------- a. the shape sweep
def test_a_rows_shape_of_the_sweep_leaves_idle_waves_in_its_last_workgroup():
    """S * N is no multiple of 4 for at least one rows shape: the last workgroup's waves beyond
    the last row must return without a store."""
    idle = [(N, W, F) for N, W, F, form in SWEEP if form == "rows" and (len(_ts(W)) * B * N) % 4]
    assert (3, 13, 5) in idle and len(idle) >= 4, idle


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("N,W,F,form", SWEEP, ids=IDS)
def test_shape_sweep_against_the_data_model(N, W, F, form, ring):
    c = _case(N, W, F)
    S, T, shape = c.S, c.T, (c.S, N, W, F)
    assert S == B * len(_ts(W)) and T == 2 * W + 3 and c.Ts == W + T + 6
    _assert_names(N, W, F, S, form)
    # the lockstep entry point against lockstep_ref
    lock_d = _run(functools.partial(gather_lockstep, c.series, N, W, c.start_d, c.weights_d, T, B, ring, c.t_d, c.e_d,
                                    F=F), shape)
    lock = lock_d.cpu().numpy()
    outside = _assert_nan_outside(lock, c.start[c.e] + c.t, c.Ts, F)
    at_t0 = outside[c.t == 0]                                  # envs 0 .. 4 in order
    if W >= 3:                                                 # W = 1: a window is wholly inside or wholly outside
        assert at_t0[0].all() and at_t0[1].any() and not at_t0[1].all() and not at_t0[2].any()
    assert at_t0[3].all() and not outside[c.e == 4].any() and outside[(c.e == 2) & (c.t >= 2)].any(1).all()
    _assert_bits(lock, _lockstep_want(N, W, F, ring), f"lockstep {ring}")
    # the env entry point fed lockstep bookkeeping: the same bytes, carry = 0 and carry = W zero rows in front
    first, updates = _i32(c.first_lock), _i32(c.updates_lock)
    got = _run(functools.partial(gather_env, c.series, N, W, first, updates, c.weights_d, 0, T, B, ring, c.t_d, c.e_d,
                                 F=F), shape)
    assert torch.equal(_canon_d(got), _canon_d(lock_d)), "env form, lockstep bookkeeping, carry = 0"
    shifted = torch.cat([torch.zeros(W, B, N, device=DEV), c.weights_d]).contiguous()
    got = _run(functools.partial(gather_env, c.series, N, W, first, updates, shifted, W, T, B, ring, c.t_d, c.e_d,
                                 F=F), shape)
    assert torch.equal(_canon_d(got), _canon_d(lock_d)), "env form, lockstep bookkeeping, carry = W"
    # the env entry point on bookkeeping of its own against window_ref
    for carry in (0, W):
        k = _books(N, W, F, carry)
        got = _run(functools.partial(gather_env, c.series, N, W, k.first_d, k.updates_d, k.weights_d, carry, T, B, ring,
                                     c.t_d, c.e_d, F=F), shape).cpu().numpy()
        outside = _assert_nan_outside(got, k.first[c.t, c.e], c.Ts, F)
        assert outside[c.e == 0].any(1).all() and outside[c.e == 1].any(1).all()        # off both ends
        assert outside[(c.e == 3) & (c.t == T)].all() and not outside[c.e == 4].any()
        assert (k.updates[c.t, c.e] <= c.t + carry)[c.e != 2].all() and (k.updates[c.t, 2] > c.t + carry).all()
        _assert_bits(got, _env_want(N, W, F, ring, carry), f"env {ring} carry={carry}")


# ---------------------------------------------------------------- b. alignment
@pytest.mark.parametrize("aligned", [2, 1, 0], ids=["s+4B", "series+4B", "both+4B"])
@pytest.mark.parametrize("N,W", [(8, 32), (63, 52)], ids=["8x32", "63x52"])
def test_misaligned_pointers_take_the_rows_kernels_and_give_the_same_bytes(N, W, aligned):
    F = 5
    c, k = _case(N, W, F), _books(N, W, F, W)
    S, T, shape = c.S, c.T, (c.S, N, W, F)
    _assert_names(N, W, F, S, "tile")
    _assert_names(N, W, F, S, "rows", aligned=aligned)
    s_off = 0 if aligned & 1 else 1
    series = c.series
    if not aligned & 2:                                       # a view into a larger buffer, 4 B past a 16-B boundary
        raw_series = torch.full((c.bars.size + 8,), float("inf"), device=DEV)
        view = raw_series[1:1 + c.bars.size]
        view.copy_(c.series.bars.reshape(-1))
        series = types.SimpleNamespace(bars=view.view(c.Ts, N, F - 1))
        assert series.bars.data_ptr() % 16 == 4 and series.bars.is_contiguous()
    for ring in RINGS:
        def lock(m, out):
            return gather_lockstep(m, N, W, c.start_d, c.weights_d, T, B, ring, c.t_d, c.e_d, out=out, F=F)

        def env(m, out):
            return gather_env(m, N, W, k.first_d, k.updates_d, k.weights_d, W, T, B, ring, c.t_d, c.e_d, out=out, F=F)

        for fn, want, what in ((lock, _lockstep_want(N, W, F, ring), "lockstep"),
                               (env, _env_want(N, W, F, ring, W), "env")):
            tile = _run(functools.partial(fn, c.series), shape)           # both pointers aligned: the tile form
            rows = _run(functools.partial(fn, series), shape, off=s_off)
            assert rows.data_ptr() % 16 == 4 * s_off
            assert torch.equal(_canon_d(rows), _canon_d(tile)), f"{what} {ring}: the rows form's bytes differ"
            _assert_bits(rows.cpu().numpy(), want, f"{what} {ring} aligned={aligned}")


# ---------------------------------------------------------------- c. the store policy
def test_the_nt_and_the_sc1_tile_kernels_write_the_same_windows():
    """(63, 52, 5): 2,048 samples are 134,184,960 B of windows, at most 128 MiB, and take <16>;
    2,049 are 134,250,480 B and take <2>. One call of 2,049 against two of 1,024 and 1,025."""
    N, W, F, S = 63, 52, 5, 2049
    per = N * W * F
    assert 2048 * per * 4 == 134_184_960 <= 128 << 20 < 2049 * per * 4 == 134_250_480
    _assert_names(N, W, F, 2048, "tile", policy=16)
    _assert_names(N, W, F, 2049, "tile", policy=2)
    _assert_names(N, W, F, 1024, "tile", policy=16)
    _assert_names(N, W, F, 1025, "tile", policy=16)
    c, k = _case(N, W, F), _books(N, W, F, W)
    T = c.T
    rng = np.random.default_rng(2049)
    t = np.concatenate([c.t, rng.integers(0, T + 1, S - c.S)])           # the sweep's edge samples first
    e = np.concatenate([c.e, rng.integers(0, B, S - c.S)])
    t_d, e_d = _i32(t), _i32(e)
    check = np.concatenate([[0, S - 1], np.random.default_rng(30).choice(np.arange(1, S - 1), 30, replace=False)])
    check_d = torch.as_tensor(check, device=DEV)
    ring = "storage"

    def lock(ti, ei, out):
        return gather_lockstep(c.series, N, W, c.start_d, c.weights_d, T, B, ring, ti, ei, out=out, F=F)

    def env(ti, ei, out):
        return gather_env(c.series, N, W, k.first_d, k.updates_d, k.weights_d, W, T, B, ring, ti, ei, out=out, F=F)

    def lock_ref(t_, b_):
        return lockstep_ref(c.bars, c.start, c.weights, W, ring, t_, b_)

    def env_ref(t_, b_):
        return window_ref(c.bars, k.first, k.updates, k.weights, W, W, ring, t_, b_)

    for fn, ref, what in ((lock, lock_ref, "lockstep"), (env, env_ref, "env")):
        raw, view = _guarded(S * per)
        fn(t_d, e_d, view)                                                # one call: <2>
        _assert_guards(raw, S * per)
        one = view.view(S, N, W, F)
        raw2, view2 = _guarded(S * per)
        two = view2.view(S, N, W, F)
        assert two[1024:].data_ptr() % 16 == 0
        fn(t_d[:1024].contiguous(), e_d[:1024].contiguous(), two[:1024])  # two calls: <16> each
        fn(t_d[1024:].contiguous(), e_d[1024:].contiguous(), two[1024:])
        _assert_guards(raw2, S * per)
        assert torch.equal(_canon_d(one), _canon_d(two)), f"{what}: <2> and <16> differ"
        got = one[check_d].cpu().numpy()
        want = np.stack([ref(int(t[j]), int(e[j])) for j in check])
        _assert_bits(got, want, f"{what} <2>")
        del raw, raw2, view, view2, one, two


# ---------------------------------------------------------------- d. the buffer with F != 5
def _feature_series(B_, N, W, T, F):
    from pmenv import MarketSeries
    rng = np.random.default_rng(B_ + N + W + F)
    bars = (100 * np.exp(0.01 * rng.standard_normal((W + T + 40, N, F - 1)).cumsum(0))).astype(np.float32)
    return MarketSeries(bars, device=DEV)


def _feature_env(B_, N, W, F, ring):
    from pmenv import TradingEnv
    return TradingEnv(num_envs=B_, num_assets=N, window=W, features=F, device=DEV, ring=ring, track_info=False,
                      close_channel=F - 2)


def _all_pairs(T, B_):
    tt = torch.arange(1, T + 1, device=DEV).repeat_interleave(B_)
    ee = torch.arange(B_, device=DEV).repeat(T)
    return tt, ee


BUFFER_SHAPES = [(9, 3, 6, 8), (9, 6, 10, 3)]
BUFFER_IDS = ["F8", "F3"]


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("B_,N,W,F", BUFFER_SHAPES, ids=BUFFER_IDS)
def test_lockstep_buffer_rematerialises_windows_of_other_channel_counts(B_, N, W, F, ring):
    from pmenv.rollout_buffer import DeviceRolloutBuffer
    T = 2 * W + 3
    _assert_names(N, W, F, B_, "rows")
    _assert_names(N, W, F, T * B_, "rows")
    m = _feature_series(B_, N, W, T, F)
    env = _feature_env(B_, N, W, F, ring)
    buf = DeviceRolloutBuffer(B_, N, W, T, features=F, device=DEV, close_channel=F - 2, series=m, ring=ring)
    start = m.random_starts(B_, W, T, generator=torch.Generator().manual_seed(F))
    buf.reset(start=start)
    obs = m.initial_window(start, W)
    env.reset(obs)
    held = [obs.clone()]
    assert obs.shape == (B_, N, W, F) and torch.equal(_canon_d(buf.obs(0)), _canon_d(obs))
    w = torch.empty(B_, N, device=DEV)
    g = torch.Generator().manual_seed(W)
    for t in range(1, T + 1):
        a = torch.softmax(torch.randn(B_, N, generator=g).to(DEV), -1)
        r, _ = env.step(a, obs, series=m, day=start + W + t - 1, weights_out=w)
        buf.add(a, env.value, r, weights=w)
        assert torch.equal(_canon_d(buf.obs(t)), _canon_d(obs)), f"window after {t} steps"
        held.append(obs.clone())
    assert not bool(torch.isnan(obs).any()) and float(obs[..., F - 1].abs().sum()) > 0
    tt, ee = _all_pairs(T, B_)
    s = buf.gather(tt, ee)[0]
    assert s.shape == (T * B_, N, W, F)
    want = torch.stack([held[t - 1][b] for t, b in zip(tt.tolist(), ee.tolist())])
    assert torch.equal(_canon_d(s), _canon_d(want))


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("B_,N,W,F", BUFFER_SHAPES, ids=BUFFER_IDS)
def test_episodes_buffer_rematerialises_windows_of_other_channel_counts(B_, N, W, F, ring):
    from pmenv import Episodes
    from pmenv.rollout_buffer import DeviceRolloutBuffer
    T = 2 * W + 3
    _assert_names(N, W, F, B_, "rows")
    _assert_names(N, W, F, T * B_, "rows")
    m = _feature_series(B_, N, W, T, F)
    start, restart, length = _roles(B_, W, T, np.random.default_rng(B_ * W + F))
    ep = Episodes(m, W, start, restart=restart, length=length)
    env = _feature_env(B_, N, W, F, ring)
    buf = DeviceRolloutBuffer(B_, N, W, T, features=F, device=DEV, close_channel=F - 2, series=m, ring=ring,
                              episodes=True)
    buf.reset(start=ep.start)
    obs = m.initial_window(ep.start, W)
    env.reset(obs)
    held = [obs.clone()]
    assert torch.equal(_canon_d(buf.obs(0)), _canon_d(obs))
    clones, _, dones = _drive(buf, env, m, ep, obs, T, torch.Generator().manual_seed(F))
    held += clones
    done = torch.stack(dones).bool().cpu().numpy()
    assert done[:, 0].all() and done[:, 3].sum() == 1 and not done[:, 4].any()      # restarts, and an env without
    assert int(buf.updates[:, 4].max()) == T >= 2 * W                          # two wraps inside one episode
    for t in range(1, T + 1):
        assert torch.equal(_canon_d(buf.obs(t)), _canon_d(held[t])), f"window after {t} steps"
    tt, ee = _all_pairs(T, B_)
    s = buf.gather(tt, ee)[0]
    want = torch.stack([held[t - 1][b] for t, b in zip(tt.tolist(), ee.tolist())])
    assert torch.equal(_canon_d(s), _canon_d(want))
