"""Per-env episodes on the resident series (pmenv_restart_days, TradingEnv.restart,
pmenv.episodes): bitwise against the composition it replaces (pmenv_window_init_days, a
masked copy, pmenv_reset(mask)), against the CPU oracle per episode, under hipGraph
replay, and its argument checks. Needs an MI355X."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from episode_ref import restart_ref, window_ref
from oracle import OracleEnv, gae as or_gae

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FAR = 1 << 30          # an end no env reaches


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _bits(x):
    return x.contiguous().view(torch.int32 if x.element_size() == 4 else torch.int64)


def _series(T, N, F, seed):
    """A [T, N, F-1] random walk (every channel a jittered close) as (MarketSeries, numpy)."""
    from pmenv import MarketSeries
    rng = np.random.default_rng(seed)
    closes = 100 * np.exp(np.cumsum(0.01 * rng.standard_normal((T, N)), axis=0))
    ser = np.empty((T, N, F - 1), np.float32)
    for f in range(F - 1):
        ser[..., f] = closes * np.exp(0.002 * rng.standard_normal(closes.shape))
    ser[..., min(3, F - 2)] = closes
    return MarketSeries(ser, device=DEV), ser


def _env(B, N, W, F, impl="auto"):
    from pmenv import TradingEnv
    return TradingEnv(num_envs=B, num_assets=N, window=W, features=F, device=DEV, track_info=False, step_impl=impl)


# (B, N, W, F, step_impl): each shape one way the kernel can go wrong
SHAPES = [
    (1, 5, 50, 5, "auto"),          # B below one slice; the tiny step
    (67, 30, 50, 5, "auto"),        # a slice tail
    (130, 7, 10, 3, "auto"),        # F != 5; env window of 210 floats, not 16-B granular
    (64, 32, 32, 8, "auto"),        # F = 8, exactly one slice
    (3, 129, 50, 5, "auto"),        # N > 64
    (2, 200, 50, 5, "auto"),        # a 160 KB series slab: the fallback form at F = 5
    (256, 30, 50, 5, "flat"),
    (256, 30, 50, 5, "relay"),
    (256, 30, 50, 5, "two_launch"),
    (256, 30, 50, 5, "one_launch"),
]
NAN_SHAPE = (67, 30, 50, 5, "auto")     # one env restarts past the series' end here (mask "all")


def _tail(B):
    return np.arange(B) >= 64 * ((B - 1) // 64)


MASKS = {
    "none": lambda B: np.zeros(B, bool),
    "all": lambda B: np.ones(B, bool),
    "first": lambda B: np.arange(B) == 0,
    "last": lambda B: np.arange(B) == B - 1,
    "alternate": lambda B: np.arange(B) % 2 == 0,
    "tail": _tail,
}


def _stepped_pair(B, N, W, F, impl):
    """Two handles of one config on one series, stepped W + 3 times with the same Philox
    actions (past the ring's wrap: counter, ring and value are not the reset state)."""
    from pmenv import synth
    T = 6 * W + 30
    ms, ser = _series(T, N, F, seed=B * 131 + N)
    rng = np.random.default_rng(B + 7 * W)
    start = rng.integers(0, W + 1, B)
    restart = rng.integers(0, W + 1, B)
    K = W + 3
    act = synth.actions(K + 2 * W, B, N, seed=7, device=DEV)
    start_t = _t(start, torch.int32)
    envs, obss = [], []
    for _ in range(2):
        env = _env(B, N, W, F, impl)
        obs = ms.initial_window(start_t, W)
        env.reset(obs)
        day = start_t + W
        for i in range(K):
            env.step(act[i], obs, series=ms, day=day)
            day = day + 1
        envs.append(env)
        obss.append(obs)
    last = start + W + K - 1                      # the bar the last step appended
    return ms, ser, T, start, restart, act, envs, obss, last


@pytest.mark.parametrize("mask_name", list(MASKS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restart_equals_the_composition_bitwise(shape, mask_name):
    from pmenv import Episodes
    B, N, W, F, impl = shape
    ms, ser, T, start, restart, act, (ea, eb), (oa, ob), last = _stepped_pair(B, N, W, F, impl)
    K = W + 3
    want = MASKS[mask_name](B)
    ep = Episodes(ms, W, start, restart=restart)
    if shape == NAN_SHAPE and mask_name == "all":
        restart = restart.copy()
        restart[5] = T - W + 2                    # its last two days lie outside the series: NaN
        ep.restart.copy_(_t(restart, torch.int32))
    end = np.where(want, last + 1, FAR)
    ep.next_day.copy_(_t(last, torch.int32))
    ep.end.copy_(_t(end, torch.int32))
    mask, new_day = restart_ref(last, end, restart, W)
    assert np.array_equal(mask, want)

    nf0 = ea.nonfinite_count()
    done = ea.restart(oa, ep)                     # handle A: one launch
    assert done is ep.done

    mask_t = _t(mask, torch.bool)                 # handle B: what the parent composes
    restart_t = _t(restart, torch.int32)
    full = ms.initial_window(restart_t, W)
    ob[mask_t] = full[mask_t]
    eb.reset(ob, mask=mask_t)
    day_b = torch.where(mask_t, restart_t + W, _t(last, torch.int32) + 1)

    assert np.array_equal(done.cpu().numpy().astype(bool), mask)
    assert torch.equal(ep.next_day, day_b) and np.array_equal(day_b.cpu().numpy(), new_day)
    assert torch.equal(_bits(oa), _bits(ob)), "windows differ"
    if shape == NAN_SHAPE and mask_name == "all":
        assert np.array_equal(np.isnan(oa[5].cpu().numpy()), np.isnan(window_ref(ser, restart[5:6], W, F)[0]))
        assert torch.isnan(oa[5, :, W - 2:, :F - 1]).all() and not torch.isnan(oa[5, :, :W - 2]).any()
    assert torch.equal(ea._state, eb._state), "state blobs differ"
    assert ea.nonfinite_count() == nf0

    # 2W more steps: a stale snapshot or halo of the flat / relay step would show here
    ep.end.fill_(FAR)
    for i in range(K, K + 2 * W):
        ra, _ = ea.step(act[i], oa, series=ms, day=ep.next_day)
        rb, _ = eb.step(act[i], ob, series=ms, day=day_b)
        assert not ea.restart(oa, ep).any()
        day_b = day_b + 1
        assert torch.equal(_bits(ra), _bits(rb)), f"reward differs at step {i}"
        assert torch.equal(_bits(ea.value), _bits(eb.value)), f"value differs at step {i}"
        assert torch.equal(_bits(oa), _bits(ob)), f"window differs at step {i}"
    assert torch.equal(ep.next_day, day_b)
    assert torch.equal(ea._state, eb._state)


@pytest.mark.parametrize("shape", SHAPES[:6], ids=lambda s: "x".join(map(str, s)))
def test_envs_that_do_not_restart_are_untouched(shape):
    from pmenv import Episodes
    B, N, W, F, impl = shape
    ms, ser, T, start, restart, act, (ea, _), (oa, _), last = _stepped_pair(B, N, W, F, impl)
    mask = MASKS["alternate"](B)
    keep = _t(~mask, torch.bool)
    ep = Episodes(ms, W, start, restart=restart)
    ep.next_day.copy_(_t(last, torch.int32))
    ep.end.copy_(_t(np.where(mask, last + 1, FAR), torch.int32))
    win0 = oa.clone()
    fields = ("_value", "_stat_a", "_stat_b", "_counter", "_ring", "_last_close", "_w_new")
    before = {f: getattr(ea, f).clone() for f in fields}
    nf0 = ea._nonfinite.clone()
    ea.restart(oa, ep)
    assert torch.equal(_bits(oa[keep]), _bits(win0[keep]))
    for f in fields:
        assert torch.equal(_bits(getattr(ea, f)[keep]), _bits(before[f][keep])), f
    assert torch.equal(ea._nonfinite, nf0)
    if mask.any():                                # and the others did change
        m = _t(mask, torch.bool)
        assert (ea._counter[m] == 0).all() and (ea._value[m] == ea.cfg.init_cash).all()
        assert np.array_equal(oa[m].cpu().numpy(), window_ref(ser, restart[mask], W, F))


@pytest.mark.parametrize("shape", [(67, 30, 50, 5), (130, 7, 10, 3)], ids=lambda s: "x".join(map(str, s)))
def test_collect_matches_the_oracle_per_episode(shape):
    """episodes.collect for 3L steps with per-env lengths L-2 .. L+2: every episode's rewards
    against an OracleEnv reset on that episode's window and stepped with the same actions
    (the tolerances of test_gpu_parity._run_both), dones against restart_ref iterated on the
    host, and rollout.gae over the per-env dones against the oracle's gae per segment."""
    from pmenv import Episodes, episodes, rollout, synth
    from pmenv.config import EnvConfig
    B, N, W, F = shape
    Fm = F - 1
    L = W + 5
    steps = 3 * L
    T = 2 * W + L + 40
    ms, ser = _series(T, N, F, seed=B + N)
    rng = np.random.default_rng(B * 3 + W)
    start = rng.integers(0, W + 1, B)
    restart = rng.integers(0, W + 31, B)
    length = rng.integers(L - 2, L + 3, B)
    act = synth.actions(steps, B, N, seed=11, device=DEV)
    cfg = EnvConfig(num_envs=B, num_assets=N, window=W, features=F, close_channel=min(3, F - 2))
    from pmenv import TradingEnv
    env = TradingEnv(config=cfg, device=DEV, track_info=False)
    ep = Episodes(ms, W, start, restart=restart, length=length)
    obs = ms.initial_window(ep.start, W)
    env.reset(obs)
    rewards, dones = episodes.collect(env, ms, ep, obs, steps, act=act)
    assert rewards.shape == (steps, B) and dones.shape == (steps, B) and dones.dtype == torch.bool
    g_r, g_d, act_h = rewards.cpu().numpy(), dones.cpu().numpy(), act.cpu().numpy()

    cenv = OracleEnv(cfg)
    cobs = window_ref(ser, start, W, F)
    cenv.reset(cobs)
    day, end = start + W, start + W + length
    for t in range(steps):
        cr, _, _ = cenv.step(act_h[t], cobs, bar=ser[day])
        err = np.abs(g_r[t].astype(np.float64) - cr)
        assert np.all(err <= 1e-6 * np.abs(cr) + 1e-9), f"step {t}: reward err {err.max():.3e}"
        done, day = restart_ref(day, end, restart, W)
        assert np.array_equal(g_d[t], done), f"dones differ at step {t}"
        if done.any():                            # a new episode: the oracle reset on its window
            cobs[done] = window_ref(ser, restart[done], W, F)
            cenv.reset(cobs, mask=done)
            end = np.where(done, restart + W + length, end)
    assert g_d.sum(0).min() >= 2                  # every env ran through at least two restarts
    assert np.array_equal(ep.next_day.cpu().numpy(), day) and np.array_equal(ep.end.cpu().numpy(), end)
    go = obs.cpu().numpy()
    assert np.array_equal(go[..., :Fm], cobs[..., :Fm])
    np.testing.assert_allclose(go[..., Fm], cobs[..., Fm], rtol=2e-7, atol=1e-12)
    np.testing.assert_allclose(env.value.cpu().numpy(), cenv.value, rtol=1e-12)
    assert np.array_equal(env._counter.cpu().numpy(), cenv.k)
    np.testing.assert_allclose(env._ring.cpu().numpy(), cenv.ring, rtol=2e-7, atol=1e-12)
    assert env.nonfinite_count() == 0

    values = _t(rng.standard_normal((steps + 1, B)))
    adv, ret = rollout.gae(rewards, values, dones, 0.99, 0.95)
    v_h = values.cpu().numpy()
    oadv, oret = np.empty_like(g_r), np.empty_like(g_r)
    for b in range(B):                            # the oracle's gae, one call per episode segment
        s = 0
        for e in list(np.flatnonzero(g_d[:, b])) + [steps - 1]:
            if e < s:
                continue
            v = v_h[s:e + 2, b:b + 1].copy()
            if g_d[e, b]:
                v[-1] = 0.0                       # the episode ended: nothing to bootstrap from
            a, r = or_gae(g_r[s:e + 1, b:b + 1], v, None, 0.99, 0.95)
            oadv[s:e + 1, b], oret[s:e + 1, b] = a[:, 0], r[:, 0]
            s = e + 1
    np.testing.assert_allclose(adv.cpu().numpy(), oadv, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ret.cpu().numpy(), oret, rtol=1e-5, atol=1e-5)


def test_step_and_restart_replay_from_a_captured_graph():
    """[step, restart] captured once at 256 x 30 x 50 x 5 (flat, in place) with a static
    action, replayed until every env restarted: bit-equal to an eager handle."""
    from pmenv import Episodes, _abi
    B, N, W, F = 256, 30, 50, 5
    T = 3 * W + 40
    ms, ser = _series(T, N, F, seed=5)
    rng = np.random.default_rng(9)
    start = rng.integers(0, W + 1, B)
    restart = rng.integers(0, W + 1, B)
    length = 3 + np.arange(B) % 8                 # staggered 3 .. 10
    act = torch.softmax(torch.randn(B, N, device=DEV, generator=torch.Generator(DEV).manual_seed(3)), -1)
    lib = _abi.load()
    eg, ee = _env(B, N, W, F, "flat"), _env(B, N, W, F, "flat")
    epg = Episodes(ms, W, start, restart=restart, length=length)
    epe = Episodes(ms, W, start, restart=restart, length=length)
    og, oe = ms.initial_window(epg.start, W), ms.initial_window(epe.start, W)
    eg.reset(og)
    ee.reset(oe)
    rew = torch.empty(B, device=DEV)
    args = _abi.PmenvStepArgs()
    args.action, args.bar, args.day, args.series_days = act.data_ptr(), ms.bars.data_ptr(), epg.next_day.data_ptr(), T
    args.obs, args.reward = og.data_ptr(), rew.data_ptr()
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()                                  # no collection (frees) inside the capture
    gc.disable()
    try:
        with torch.cuda.graph(g):
            s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _abi.check(lib.pmenv_step_ex(eg._h, ctypes.byref(args), s), eg._h)
            _abi.check(lib.pmenv_restart_days(eg._h, p(og), p(ms.bars), T, p(epg.next_day), p(epg.end),
                                              p(epg.restart), p(epg.done), s), eg._h)
            epg._restarted()
    finally:
        gc.enable()
    assert "device-sequenced" in eg.step_path
    seen = torch.zeros(B, dtype=torch.bool, device=DEV)
    for _ in range(12):
        g.replay()
        re, _ = ee.step(act, oe, series=ms, day=epe.next_day)
        seen |= ee.restart(oe, epe).bool()
        assert torch.equal(epg.done, epe.done)
        assert torch.equal(_bits(rew), _bits(re))
    assert seen.all()
    assert torch.equal(_bits(og), _bits(oe))
    assert torch.equal(_bits(eg.value), _bits(ee.value))
    assert torch.equal(epg.next_day, epe.next_day) and torch.equal(epg.end, epe.end)
    assert torch.equal(eg._state, ee._state)


def test_arguments():
    from pmenv import Episodes, TradingEnv, _abi
    B, N, W, F = 3, 5, 8, 5
    ms, _ = _series(40, N, F, seed=1)
    env = _env(B, N, W, F)
    ep = Episodes(ms, W, [0, 1, 2])
    obs = ms.initial_window(ep.start, W)
    env.reset(obs)
    lib = _abi.load()
    ptrs = [obs, ms.bars, ep.next_day, ep.end, ep.restart, ep.done]
    names = ["obs", "series", "day", "end", "restart", "done"]
    for i, name in enumerate(names):
        a = [ctypes.c_void_p(t.data_ptr()) for t in ptrs]
        a[i] = None
        rc = lib.pmenv_restart_days(env._h, a[0], a[1], 40, a[2], a[3], a[4], a[5], None)
        assert rc == -1, name                      # PMENV_ERR_ARG
        assert name in lib.pmenv_last_error(env._h).decode()
    assert lib.pmenv_restart_days(None, *[ctypes.c_void_p(t.data_ptr()) for t in ptrs[:2]], 40,
                                  *[ctypes.c_void_p(t.data_ptr()) for t in ptrs[2:]], None) == -1
    with pytest.raises(ValueError, match="device window"):
        env.restart(obs.cpu(), ep)
    with pytest.raises(ValueError, match="batched"):
        _env(1, N, W, F).restart(obs[0], Episodes(ms, W, [0]))
    tracked = TradingEnv(num_envs=B, num_assets=N, window=W, features=F, device=DEV, track_info=True)
    tracked.reset(obs)
    with pytest.raises(ValueError, match="info"):
        tracked.restart(obs, ep)
    assert env.restart(obs, ep) is ep.done and ep.next_day.tolist() == [W + 1, W + 2, W + 3]
