"""The compact rollout's per-env form on an MI355X (pmenv_rollout_gather_env,
DeviceRolloutBuffer(episodes=True), OnPolicy(episodes=True)): bitwise against the lockstep
gather on lockstep bookkeeping, against the windows the envs themselves hold across restarts
and resumed rollouts, against a numpy restatement of the data model (include/pmenv.h) for
days outside the series and out-of-contract update counts, under hipGraph replay, and its
argument checks. Needs a GPU."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from rollout_window_ref import window_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (B, N, W, T), the form each takes
SHAPES = [(5, 30, 50, 60, "tile"),       # the shape the lockstep test uses
          (8, 4, 4, 14, "tile"),         # the tile at its smallest (N*W*5 % 4 == 0)
          (33, 7, 6, 20, "rows"),
          (64, 1, 2, 9, "rows")]         # W = 2, one asset
IDS = ["x".join(map(str, s[:4])) for s in SHAPES]
RINGS = ["storage", "chrono"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


def _p(x):
    return ctypes.c_void_p(x.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _i32(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int32, device=DEV)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _series(B, N, W, T, extra=40):
    """The series of test_gpu_compact_rollout_rematerialises_the_env_windows: W + T + 40 days."""
    from pmenv import MarketSeries
    rng = np.random.default_rng(B + N + W)
    Ts = W + T + extra
    bars = (100 * np.exp(0.01 * rng.standard_normal((Ts, N, 4)).cumsum(0))).astype(np.float32)
    return MarketSeries(bars, device=DEV), bars


def _assert_form(N, W, S, form):
    from pmenv import _abi
    from pmenv.replay import gather_path
    env_path = _abi.load().pmenv_rollout_gather_env_path(N, 5, W, S, 3).decode()
    assert env_path.startswith(f"rollout_gather_env_{form}_kernel"), env_path
    lock = gather_path("rollout", N, W, S=S)
    assert lock.startswith(f"rollout_gather_{form}_kernel"), lock
    assert env_path.split(" ")[1:] == lock.split(" ")[1:]            # the same plan


def gather_env(m, N, W, first, updates, weights, carry, T_rec, B, ring, ti, ei, out=None, F=5):
    """pmenv_rollout_gather_env through the raw ABI; m: anything with the series as .bars [Ts, N, F-1]
    (a view too); out: the [S, N, W, F] floats to write (a view too), a fresh tensor if None."""
    from pmenv import _abi
    S = ti.numel()
    if out is None:
        out = torch.empty(S, N, W, F, device=DEV)
    _abi.check(_abi.load().pmenv_rollout_gather_env(_p(m.bars), m.bars.shape[0], N, F, W, _p(first), _p(updates),
                                                    _p(weights), carry, T_rec, B, _abi.RING_MODES[ring], _p(ti),
                                                    _p(ei), S, _p(out), _stream()), None, "pmenv_rollout_gather_env")
    return out


def gather_lockstep(m, N, W, start, weights, T_rec, B, ring, ti, ei, out=None, F=5):
    """pmenv_rollout_gather through the raw ABI; m, out, F as gather_env's."""
    from pmenv import _abi
    S = ti.numel()
    if out is None:
        out = torch.empty(S, N, W, F, device=DEV)
    _abi.check(_abi.load().pmenv_rollout_gather(_p(m.bars), m.bars.shape[0], N, F, W, _p(start), _p(weights), T_rec, B,
                                                _abi.RING_MODES[ring], _p(ti), _p(ei), S, _p(out), _stream()))
    return out


def _pairs(ts, B):
    ti = torch.tensor([t for t in ts for _ in range(B)], dtype=torch.int32, device=DEV)
    ei = torch.arange(B, dtype=torch.int32, device=DEV).repeat(len(ts))
    return ti, ei


# ---------------------------------------------------------------- 1. lockstep equivalence
@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("B,N,W,T,form", SHAPES, ids=IDS)
def test_lockstep_bookkeeping_gives_the_lockstep_gathers_bytes(ring, B, N, W, T, form):
    m, _ = _series(B, N, W, T)
    ts = sorted({0, 1, W - 2, W - 1, W, T})
    ti, ei = _pairs(ts, B)
    _assert_form(N, W, ti.numel(), form)
    g = torch.Generator().manual_seed(B + W)
    start = m.random_starts(B, W, T, generator=g)
    w = torch.softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
    first = (start[None, :] + torch.arange(T + 1, dtype=torch.int32, device=DEV)[:, None]).contiguous()
    updates = torch.arange(T + 1, dtype=torch.int32, device=DEV)[:, None].repeat(1, B).contiguous()
    want = gather_lockstep(m, N, W, start, w, T, B, ring, ti, ei)
    assert not bool(torch.isnan(want).any())
    got = gather_env(m, N, W, first, updates, w, 0, T, B, ring, ti, ei)
    assert torch.equal(_bits(got), _bits(want))
    shifted = torch.cat([torch.zeros(W, B, N, device=DEV), w]).contiguous()      # carry = W zero rows in front
    got = gather_env(m, N, W, first, updates, shifted, W, T, B, ring, ti, ei)
    assert torch.equal(_bits(got), _bits(want))


# ---------------------------------------------------------------- 2. the envs' own windows
def _roles(B, W, T, rng):
    """Episode lengths per env: 1 (restarts after every step), W-1 and W (the ring just does
    not fill / just fills), T (> W here: the storage-order wrap inside an episode, and the
    episode ends exactly at step T), one that never ends, the rest random."""
    assert T > W and B >= 5
    length = np.concatenate([[1, max(W - 1, 1), W, T, T + 25], rng.integers(2, T + 11, B - 5)])
    start = rng.integers(0, 8, B)
    restart = start + 1 + rng.integers(0, 3, B)            # differs from start, <= 10
    return start, restart, length


def _drive(buf, env, m, ep, obs, T, g):
    """T steps of step -> add -> restart -> restarted; returns the clones of obs after every
    restart call, the appended days and the dones."""
    B, N = buf.B, buf.N
    w = torch.empty(B, N, device=DEV)
    clones, days, dones = [], [], []
    for t in range(1, T + 1):
        a = torch.softmax(torch.randn(B, N, generator=g).to(DEV), -1)
        days.append(ep.next_day.clone())
        r, _ = env.step(a, obs, series=m, day=ep.next_day, weights_out=w)
        buf.add(a, env.value, r, weights=w)
        done = env.restart(obs, ep)
        buf.restarted(done, ep.next_day)
        clones.append(obs.clone())
        dones.append(done.clone())
    return clones, days, dones


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("B,N,W,T,form", SHAPES, ids=IDS)
def test_buffer_rematerialises_the_windows_of_envs_that_restart(ring, B, N, W, T, form):
    from pmenv import Episodes, TradingEnv
    from pmenv.rollout_buffer import DeviceRolloutBuffer
    m, bars = _series(B, N, W, T)
    _assert_form(N, W, B, form)
    rng = np.random.default_rng(B * W)
    start, restart, length = _roles(B, W, T, rng)
    ep = Episodes(m, W, start, restart=restart, length=length)
    env = TradingEnv(num_envs=B, num_assets=N, window=W, device=DEV, ring=ring, track_info=False)
    buf = DeviceRolloutBuffer(B, N, W, T, device=DEV, series=m, ring=ring, episodes=True)
    # a [T + 1] and w [W + T] rows of B * N floats, 21 B of v / r / first / updates / done per (row, env)
    assert buf.nbytes() < 4 * (2 * T + W + 2) * B * N + 24 * (T + 1) * B + 64 * B       # O(T * B * N)
    buf.reset(start=ep.start)
    obs = m.initial_window(ep.start, W)
    env.reset(obs)
    assert torch.equal(_bits(buf.obs(0)), _bits(obs))
    clones, days, dones = _drive(buf, env, m, ep, obs, T, torch.Generator().manual_seed(3))
    done = torch.stack(dones).bool().cpu().numpy()
    assert done[:, 0].all() and done[T - 1, 3] and done[:, 3].sum() == 1 and not done[:, 4].any()
    assert torch.equal(buf.done[1:].bool().cpu(), torch.as_tensor(done))
    assert int(buf.updates[:, 3].max()) == T - 1 >= W                     # the wrap inside an episode
    for t in range(1, T + 1):
        assert torch.equal(_bits(buf.obs(t)), _bits(clones[t - 1])), f"window after {t} steps"
        d = days[t - 1].long()
        assert torch.equal(buf.price_relatives(t), m.bars[d, :, 3] / m.bars[d - 1, :, 3]), t
    # the batch of a step right after a restart (env 0 restarts after every step) and of one
    # that is not (env 4 never restarts): _a / _v are the reset state / the recorded row
    tt = torch.tensor([3, 3, T], device=DEV)
    ee = torch.tensor([0, 4, 3], device=DEV)
    s, a_, r_, v_prev, a_prev, p = buf.gather(tt, ee)
    assert s.shape == (3, N, W, 5) and p.shape == (3, N, 1) and v_prev.shape == (3, 1, 1)
    for j, (t, b) in enumerate(zip(tt.tolist(), ee.tolist())):
        assert torch.equal(_bits(s[j]), _bits(clones[t - 2][b]))
        assert torch.equal(a_[j, :, 0], buf.a[t, b]) and float(r_[j]) == float(buf.r[t, b])
        d = int(days[t - 1][b])
        assert torch.equal(p[j, :, 0], m.bars[d, :, 3] / m.bars[d - 1, :, 3])
    e0 = torch.zeros(N, device=DEV)
    e0[0] = 1.0
    assert int(buf.updates[2, 0]) == 0 and torch.equal(a_prev[0, :, 0], e0) and float(v_prev[0]) == buf.init_cash
    assert int(buf.updates[2, 4]) == 2 and torch.equal(a_prev[1, :, 0], buf.a[2, 4])
    assert float(v_prev[1]) == float(buf.v[2, 4].float()) != buf.init_cash
    assert int(buf.updates[T - 1, 3]) == T - 1 and torch.equal(a_prev[2, :, 0], buf.a[T - 1, 3])
    # the recorded dones cut the return pass
    from pmenv.rollout import gae
    values = torch.randn(T + 1, B, device=DEV)
    adv, ret = buf.returns(values, 0.99, 0.95)
    adv2, ret2 = gae(buf.r[1:].contiguous(), values, torch.as_tensor(done, device=DEV), 0.99, 0.95)
    assert torch.equal(adv, adv2) and torch.equal(ret, ret2)


# ---------------------------------------------------------------- 3. resume
@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("B,N,W,T", [(8, 4, 4, 3), (8, 4, 4, 6), (33, 7, 6, 4), (33, 7, 6, 9)],
                         ids=["tile-T<W", "tile-T>W", "rows-T<W", "rows-T>W"])
def test_three_resumed_rollouts_keep_the_envs_windows(ring, B, N, W, T):
    from pmenv import Episodes, TradingEnv
    from pmenv.rollout_buffer import DeviceRolloutBuffer
    m, _ = _series(B, N, W, 3 * T)
    _assert_form(N, W, B, "tile" if N == 4 else "rows")
    rng = np.random.default_rng(B + T)
    start, restart, length = _roles(B, W, 3 * T, rng)
    ep = Episodes(m, W, start, restart=restart, length=length)
    env = TradingEnv(num_envs=B, num_assets=N, window=W, device=DEV, ring=ring, track_info=False)
    buf = DeviceRolloutBuffer(B, N, W, T, device=DEV, series=m, ring=ring, episodes=True)
    buf.reset(start=ep.start)
    obs = m.initial_window(ep.start, W)
    env.reset(obs)
    g = torch.Generator().manual_seed(5)
    last = obs.clone()
    for k in range(3):
        if k:
            buf.resume()
        assert len(buf) == 0
        assert torch.equal(_bits(buf.obs(0)), _bits(last)), f"row 0 of rollout {k}"
        clones, _, _ = _drive(buf, env, m, ep, obs, T, g)
        for t in range(1, T + 1):
            assert torch.equal(_bits(buf.obs(t)), _bits(clones[t - 1])), f"rollout {k}, window after {t} steps"
        last = clones[-1]
    assert int(buf.updates[T, 4]) == 3 * T                 # the env that never restarts: past t + carry for T < W


# ---------------------------------------------------------------- 4. misaligned output, days outside the series
@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("B,N,W,T,form", SHAPES, ids=IDS)
def test_against_the_data_model_outside_the_series_and_the_contract(ring, B, N, W, T, form):
    from pmenv import _abi
    m, bars = _series(B, N, W, T)
    Ts = bars.shape[0]
    rng = np.random.default_rng(B + 3 * T)
    ts = sorted({0, 1, W - 2, W - 1, W, T - 1, T})
    ti, ei = _pairs(ts, B)
    S = ti.numel()
    _assert_form(N, W, S, form)
    for carry in (0, W):
        first = rng.integers(0, Ts - W + 1, (T + 1, B))
        first[:, 0] = Ts - W + 1 + rng.integers(0, W + 3, T + 1)          # env 0: windows that run past the end
        first[T, 1] = Ts                                                # wholly outside
        tcol = np.arange(T + 1)[:, None]
        updates = rng.integers(0, tcol + carry + 1, (T + 1, B))          # in contract: <= t + carry
        updates[:, 2] = tcol[:, 0] + carry + 1 + rng.integers(0, 2 * W, T + 1)   # env 2: beyond it
        weights = rng.random((carry + T, B, N)).astype(np.float32) + 0.5
        ft, ut, wt = _i32(first), _i32(updates), torch.as_tensor(weights, device=DEV)
        got = gather_env(m, N, W, ft, ut, wt, carry, T, B, ring, ti, ei).cpu().numpy()
        below = False
        for j, (t, b) in enumerate(zip(ti.tolist(), ei.tolist())):
            want = window_ref(bars, first, updates, weights, carry, W, ring, t, b)
            assert np.array_equal(got[j].view(np.int32), want.view(np.int32)), (carry, t, b)
            outside = first[t, b] + np.arange(W) >= Ts
            assert np.array_equal(np.isnan(got[j][..., :4]).all(axis=(0, 2)), outside)
            assert np.isfinite(got[j][..., 4]).all()
            below |= b == 2 and carry + t - W < 0
        assert below == (carry == 0)             # some beyond-contract sample pointed below row 0
        # a view 4 B past a 16-B boundary takes the rows form: the same windows, nothing outside
        raw = torch.full((S * N * W * 5 + 4,), -1.0, device=DEV)
        mis = raw[1:1 + S * N * W * 5]
        assert mis.data_ptr() % 16 == 4
        assert _abi.load().pmenv_rollout_gather_env_path(N, 5, W, S, 2).startswith(b"rollout_gather_env_rows_kernel ")
        gather_env(m, N, W, ft, ut, wt, carry, T, B, ring, ti, ei, out=mis)
        assert np.array_equal(mis.view(S, N, W, 5).cpu().numpy().view(np.int32), got.view(np.int32))
        assert bool((raw[0] == -1.0) & (raw[-3:] == -1.0).all())


# ---------------------------------------------------------------- 5. OnPolicy(episodes=True)
def test_on_policy_per_env_episodes_loop():
    from pmenv import Episodes, MarketSeries, TradingEnv, episodes as episodes_mod, parallel
    from pmenv.on_policy import OnPolicy, WindowCritic, WindowPolicy
    from pmenv.rollout import gae
    B, N, W, T, Ts = 64, 30, 20, 12, 160
    rng = np.random.default_rng(11)
    bars = (100 * np.exp(0.01 * rng.standard_normal((Ts, N, 4)).cumsum(0))).astype(np.float32)
    m = MarketSeries(bars, device=DEV)
    start = rng.integers(0, 100, B)
    restart = rng.integers(0, 100, B)
    length = rng.integers(3, 10, B)

    def fresh():
        return Episodes(m, W, start, restart=restart, length=length)

    torch.manual_seed(1)
    env = TradingEnv(num_envs=B, num_assets=N, window=W, device=DEV)
    policy = WindowPolicy(W).to(DEV)
    loop = OnPolicy(env, policy, horizon=T, series=m, batch_size=B, generator=torch.Generator().manual_seed(2),
                    explore_std=0.3, episodes=True)
    with pytest.raises(ValueError):
        loop.rollout(episodes=fresh(), resume=True)                  # nothing to resume yet
    ep = fresh()
    rewards = loop.rollout(episodes=ep)
    buf = loop.buf
    assert buf.episodes and len(buf) == T and rewards.shape == (T, B)
    noise1 = loop._noise.clone()
    # an independent env fed the stored actions through episodes.collect: rewards and dones bit for bit
    ref = TradingEnv(num_envs=B, num_assets=N, window=W, device=DEV)
    rep = fresh()
    robs = m.initial_window(rep.start, W)
    ref.reset(robs)
    r_ref, d_ref = episodes_mod.collect(ref, m, rep, robs, T, act=buf.a[1:T + 1].contiguous())
    assert torch.equal(_bits(r_ref), _bits(rewards)) and torch.equal(_bits(r_ref), _bits(buf.r[1:]))
    assert torch.equal(d_ref, buf.done[1:].bool()) and bool(d_ref.any()) and not bool(d_ref.all())
    assert int(d_ref.sum(0).min()) >= 1                               # every env restarted (lengths 3-9, T = 12)
    assert torch.equal(_bits(robs), _bits(loop.obs)) and torch.equal(_bits(buf.obs(T)), _bits(robs))
    critic = WindowCritic(W).to(DEV)
    adv, ret, values = loop.advantages(critic)
    adv2, ret2 = gae(buf.r[1:].contiguous(), values, buf.done[1:].contiguous(), 0.99, 0.95)
    assert torch.equal(ret, ret2) and torch.equal(adv, parallel.normalize(adv2))
    adv_open, _ = gae(buf.r[1:].contiguous(), values, None, 0.99, 0.95)
    assert not torch.equal(adv2, adv_open)                            # the dones do cut the recursion
    w0 = [q.detach().clone() for q in policy.parameters()]
    losses = loop.update()
    assert losses.numel() == T and bool(torch.isfinite(losses).all())
    loss = loop.update_actor_critic(adv, chunk=256)
    assert np.isfinite(float(loss))
    assert any(not torch.equal(a, b) for a, b in zip(w0, policy.parameters()))
    opt = torch.optim.SGD(critic.parameters(), lr=1e-3)
    assert bool(torch.isfinite(loop.update_critic(critic, opt, ret, batch_size=B)).all())
    # a second rollout continues the envs: row 0 is the window the first one ended on
    end1 = loop.obs.clone()
    rewards2 = loop.rollout(episodes=ep, resume=True)
    assert torch.equal(_bits(buf.obs(0)), _bits(end1))
    assert not torch.equal(loop._noise, noise1)                       # keyed by the rollout counter too
    r_ref2, d_ref2 = episodes_mod.collect(ref, m, rep, robs, T, act=buf.a[1:T + 1].contiguous())
    assert torch.equal(_bits(r_ref2), _bits(rewards2)) and torch.equal(d_ref2, buf.done[1:].bool())
    assert torch.equal(_bits(buf.obs(T)), _bits(robs))
    adv, ret, values = loop.advantages(critic)
    assert bool(torch.isfinite(adv).all())


# ---------------------------------------------------------------- 6. capture
@pytest.mark.parametrize("B,N,W,T,form", SHAPES[1:3], ids=IDS[1:3])
def test_gather_env_replays_from_a_graph(B, N, W, T, form):
    m, bars = _series(B, N, W, T)
    rng = np.random.default_rng(W)
    S = 2 * B
    _assert_form(N, W, S, form)
    first = _i32(rng.integers(0, 40, (T + 1, B)))
    updates = _i32(rng.integers(0, np.arange(T + 1)[:, None] + W + 1, (T + 1, B)))
    w = torch.as_tensor(rng.random((W + T, B, N)).astype(np.float32), device=DEV)
    ti, ei = _i32(rng.integers(0, T + 1, S)), _i32(rng.integers(0, B, S))
    out = torch.zeros(S, N, W, 5, device=DEV)
    eager0 = gather_env(m, N, W, first, updates, w, W, T, B, "storage", ti, ei)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            gather_env(m, N, W, first, updates, w, W, T, B, "storage", ti, ei, out=out)
    finally:
        gc.enable()
    assert float(out.abs().sum()) == 0.0                               # captured, not run
    g.replay()
    assert torch.equal(_bits(out), _bits(eager0))
    ti.copy_(_i32(rng.integers(0, T + 1, S)))
    ei.copy_(_i32(rng.integers(0, B, S)))
    g.replay()
    eager1 = gather_env(m, N, W, first, updates, w, W, T, B, "storage", ti, ei)
    assert torch.equal(_bits(out), _bits(eager1)) and not torch.equal(_bits(eager1), _bits(eager0))


# ---------------------------------------------------------------- 7. argument errors
def test_gather_env_argument_errors_launch_nothing():
    from pmenv import _abi
    lib = _abi.load()
    B, N, W, T = 8, 4, 4, 14
    m, _ = _series(B, N, W, T)
    first = torch.zeros(T + 1, B, dtype=torch.int32, device=DEV)
    updates = torch.zeros(T + 1, B, dtype=torch.int32, device=DEV)
    w = torch.zeros(W + T, B, N, device=DEV)
    ti, ei = _pairs([0, 1], B)
    S = ti.numel()
    out = torch.full((S, N, W, 5), -7.0, device=DEV)

    def call(first=first, updates=updates, w=w, carry=W, ti=ti, ei=ei, S=S, out=out, T_rec=T, ring=0):
        q = lambda x: _p(x) if x is not None else None  # noqa: E731
        return lib.pmenv_rollout_gather_env(_p(m.bars), m.bars.shape[0], N, 5, W, q(first), q(updates), q(w), carry,
                                            T_rec, B, ring, q(ti), q(ei), S, q(out), _stream())

    ERR_ARG = -1
    for kw in (dict(first=None), dict(updates=None), dict(w=None), dict(carry=-1), dict(ti=None), dict(ei=None),
               dict(out=None), dict(S=0), dict(T_rec=-1), dict(ring=2)):
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any())
