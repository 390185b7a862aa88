"""pmenv_metrics_episodes (per-episode trajectory metrics for envs that restart on their own)
against the restatement of tests/metrics_env_ref.py, and the Python layers above it.

  ref          count and span exact (count also above the cap K), final_value bit-equal to
               values[last, b], the other fields at rtol 1e-6 / atol 1e-9 with an identical
               NaN / +-inf pattern (Sharpe under test_metrics_env_host.py's rule), unfilled
               slots NaN / {0, 0};
  lockstep     with dones = 0, slot 0 agrees with trajectory_metrics on the same arrays;
  same bits    a repeated call; the stored episodes for K = 2 and K = T; a captured call
               replayed on fresh inputs;
  isolation    a NaN touches the episode it lies in and nothing else;
  arguments    NULL pointers, K = 0, T = 0: PMENV_ERR_ARG, nothing enqueued;
  evaluate     episodes.evaluate / OffPolicy.evaluate_episodes against a manual loop.
Needs an MI355X."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import metrics_env_ref as mr
import rollout_edge_inputs as ri
from test_gpu_parity import DEV, _gpu, _t  # noqa: F401  (_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

KEYS = ("sharpe", "sortino", "max_drawdown", "average_turnover", "final_value")
RTOL, ATOL = 1e-6, 1e-9                  # test_gpu_metrics_edges_match_restatement's
ERR_ARG = -1                             # PMENV_ERR_ARG


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _unpack(got):
    out = torch.stack([got[k] for k in KEYS], 2).cpu().numpy()
    span = torch.stack([got["first"], got["last"]], 2).cpu().numpy()
    return out, span, got["count"].cpu().numpy()


def _run(ret, val, w, d, K, rf=0.04, periods=252.0, init=mr.INIT_VALUE):
    from pmenv.replay import episode_metrics
    got = episode_metrics(_t(ret, torch.float64), _t(val, torch.float64), _t(w), _t(d, torch.uint8), init, K, rf,
                          periods)
    assert got["sharpe"].dtype == torch.float64 and got["first"].dtype == torch.int32
    assert got["count"].dtype == torch.int32 and got["sharpe"].shape == (ret.shape[1], K)
    return _unpack(got)


def _compare(got, refs, K, val):
    out, span, count = got
    eo, es, ec = mr.dense(refs, K)
    assert np.array_equal(count, ec), "count"
    assert np.array_equal(span, es), "span"
    stored = np.arange(K)[None, :] < np.minimum(ec, K)[:, None]
    assert np.isnan(out[~stored]).all(), "unfilled slots"
    bi, ki = np.nonzero(stored)
    assert np.array_equal(_u64(out[bi, ki, 4]), _u64(val[span[bi, ki, 1], bi])), "final_value"
    keep = mr.sharpe_compared(refs, K)
    for i, k in enumerate(KEYS):
        m = stored & keep if i == 0 else stored
        g, e = out[..., i][m], eo[..., i][m]
        for f in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(f(g), f(e)), f"{k}: {f.__name__} pattern"
        fin = np.isfinite(e)
        np.testing.assert_allclose(g[fin], e[fin], rtol=RTOL, atol=ATOL, err_msg=k)


@pytest.mark.parametrize("kname", ["1", "2", "T"])
@pytest.mark.parametrize("rf,periods", ri.METRIC_RATES)
@pytest.mark.parametrize("T,B,N", mr.ALL_SHAPES)
def test_gpu_episode_metrics_match_restatement(T, B, N, rf, periods, kname):
    """Every (done class, value class) pair, an episode boundary on every row (B >= 9 T), T
    below the four waves, B across the 64-env blocks, and every form of the turnover part: N <= 64
    (shuffles), 64 < N <= 256 with 3, 2 and 1 envs per workgroup (metrics_env_ref.SLAB_SHAPES:
    the slab, T below and across its 8-row blocks, B no multiple of the envs per workgroup) and
    N = 257 (threads stride over the assets)."""
    K = T if kname == "T" else int(kname)
    ret, val, w, d = mr.case(T, B, N)
    got = _run(ret, val, w, d, K, rf, periods)
    _compare(got, mr.case_ref(T, B, N, rf, periods), K, val)
    if kname == "T" and B >= 9:
        assert (got[2] > 2).any() or T <= 2     # the cap is exceeded somewhere for K = 1, 2


@pytest.mark.parametrize("T,B,N", mr.ALL_SHAPES)
def test_gpu_episode_metrics_without_dones_agree_with_lockstep(T, B, N):
    from pmenv.replay import trajectory_metrics
    ret, val, w, _ = mr.case(T, B, N)
    out, span, count = _run(ret, val, w, np.zeros((T, B), np.uint8), 1)
    lock = trajectory_metrics(_t(ret, torch.float64), _t(val, torch.float64), _t(w))
    lock = torch.stack([lock[k] for k in KEYS], 1).cpu().numpy()
    assert (count == 1).all() and (span[:, 0, 0] == 1).all() and (span[:, 0, 1] == T).all()
    assert np.array_equal(_u64(out[:, 0, 4]), _u64(lock[:, 4])) and np.array_equal(_u64(lock[:, 4]), _u64(val[T]))
    for i, k in enumerate(KEYS[:4]):
        g, e = out[:, 0, i], lock[:, i]
        for f in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(f(g), f(e)), f"{k}: {f.__name__} pattern"
        fin = np.isfinite(e)
        np.testing.assert_allclose(g[fin], e[fin], rtol=RTOL, atol=ATOL, err_msg=k)


@pytest.mark.parametrize("T,B,N", [(9, 90, 3), (7, 130, 257), (64, 700, 30), (129, 1300, 4)] + mr.SLAB_SHAPES)
def test_gpu_episode_metrics_same_bits_on_every_call_and_for_every_cap(T, B, N):
    ret, val, w, d = mr.case(T, B, N)
    a = _run(ret, val, w, d, T)
    b = _run(ret, val, w, d, T)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for K in (1, 2):
        c = _run(ret, val, w, d, K)
        assert np.array_equal(_u64(c[0]), _u64(a[0][:, :K])), K
        assert np.array_equal(c[1], a[1][:, :K]) and np.array_equal(c[2], a[2]), K


@pytest.mark.parametrize("T,B,N", [(7, 130, 257), (8, 129, 30), (64, 700, 30)] + mr.SLAB_SHAPES)
def test_gpu_episode_metrics_nan_stays_in_its_episode(T, B, N):
    """A NaN in env b0's returns, values or weights leaves every other env bit-equal, and
    every other episode of env b0 too: the terminal row belongs to the episode it ends, the
    next one starts from init_value and e0. Poked: the first and the last row, a terminal
    row, row 0, envs 0 / 63 / 64 / B - 1 (lanes past B read env B - 1), asset N - 1."""
    ret, val, w, d = mr.case(T, B, N)
    d = d.copy()
    envs = (0, 63, 64, B - 1)
    e1, e2 = max(T // 3, 1), max(2 * T // 3, 2)                  # steps that end an episode
    for b0 in envs:
        d[:, b0] = 0
        d[e1 - 1, b0] = d[e2 - 1, b0] = 1
    K = 3
    base = _run(ret, val, w, d, K)
    assert all(base[1][b0].tolist() == [[1, e1], [e1 + 1, e2], [e2 + 1, T]] for b0 in envs)
    pokes = [("ret", 1), ("ret", T), ("ret", e1 + 1), ("val", 0), ("val", T), ("val", e1), ("val", e2 + 1),
             ("w", 0), ("w", T), ("w", e1), ("w", e2), ("w", e1 + 1)]
    for i, (what, row) in enumerate(pokes):
        b0 = envs[i % 4]
        r2, v2, w2 = ret.copy(), val.copy(), w.copy()
        if what == "ret":
            r2[row - 1, b0] = np.nan                             # step `row`
        elif what == "val":
            v2[row, b0] = np.nan
        else:
            w2[row, b0, N - 1] = np.nan
        k0 = 0 if row <= e1 else 1 if row <= e2 else 2           # the episode step / row `row` lies in
        got = _run(r2, v2, w2, d, K)
        keep = np.ones((B, K), bool)
        keep[b0, k0] = False
        assert np.array_equal(_u64(got[0][keep]), _u64(base[0][keep])), (what, row, b0)
        assert np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2])
        if what != "val":                                        # fmax / fmin pass a NaN value by
            assert np.isnan(got[0][b0, k0]).any(), (what, row, b0)


def _raw(lib, r, v, w, d, T, B, N, K, out, span, count, stream):
    p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    return lib.pmenv_metrics_episodes(p(r), p(v), p(w), p(d), T, B, N, mr.INIT_VALUE, 0.04, 252.0, K, p(out), p(span),
                                      p(count), stream)


def test_gpu_episode_metrics_replay_from_a_captured_graph():
    from pmenv import _abi
    lib = _abi.load()
    T, B, N, K = 9, 90, 3, 4
    ins = [mr.batch(T, B, N, seed=s) for s in (5, 6)]
    eager = [_run(*a, K) for a in ins]
    r, v = torch.zeros(T, B, dtype=torch.float64, device=DEV), torch.zeros(T + 1, B, dtype=torch.float64, device=DEV)
    w, d = torch.zeros(T + 1, B, N, device=DEV), torch.zeros(T, B, dtype=torch.uint8, device=DEV)
    out = torch.zeros(B, K, 5, dtype=torch.float64, device=DEV)
    span = torch.zeros(B, K, 2, dtype=torch.int32, device=DEV)
    count = torch.zeros(B, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()                                  # no collection (frees) inside the capture
    gc.disable()
    try:
        with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
            rc = _raw(lib, r, v, w, d, T, B, N, K, out, span, count, ctypes.c_void_p(s.cuda_stream))
    finally:
        gc.enable()
    assert rc == 0
    torch.cuda.synchronize()
    assert int(count.sum()) == 0                  # captured, not run
    for a, e in zip(ins, eager):
        for dst, src, dt in zip((r, v, w, d), a, (torch.float64, torch.float64, torch.float32, torch.uint8)):
            dst.copy_(_t(src, dt))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_u64(out.cpu().numpy()), _u64(e[0]))
        assert np.array_equal(span.cpu().numpy(), e[1]) and np.array_equal(count.cpu().numpy(), e[2])


def test_gpu_episode_metrics_argument_errors_enqueue_nothing():
    from pmenv import _abi
    from pmenv.replay import episode_metrics
    lib = _abi.load()
    T, B, N, K = 3, 5, 2, 2
    ret, val, w, d = mr.batch(T, B, N, seed=1)
    r, v, ww, dd = _t(ret, torch.float64), _t(val, torch.float64), _t(w), _t(d, torch.uint8)
    out = torch.full((B, K, 5), 7.0, dtype=torch.float64, device=DEV)
    span = torch.full((B, K, 2), 7, dtype=torch.int32, device=DEV)
    count = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    full = [r, v, ww, dd, out, span, count]
    for i in range(7):
        a = list(full)
        a[i] = None
        assert _raw(lib, a[0], a[1], a[2], a[3], T, B, N, K, a[4], a[5], a[6], st) == ERR_ARG, i
    for T_, B_, N_, K_ in [(0, B, N, K), (T, 0, N, K), (T, B, 0, K), (T, B, N, 0), (T, B, N, -1)]:
        assert _raw(lib, r, v, ww, dd, T_, B_, N_, K_, out, span, count, st) == ERR_ARG
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    assert lib.pmenv_metrics_episodes(p(r), p(v), p(ww), p(dd), T, B, N, 1.0, 0.04, 0.0, K, p(out), p(span), p(count),
                                      st) == ERR_ARG
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (span == 7).all() and (count == 7).all()
    assert _raw(lib, r, v, ww, dd, T, B, N, K, out, span, count, st) == 0
    torch.cuda.synchronize()
    assert (count >= 1).all()
    with pytest.raises(ValueError):
        episode_metrics(r, v[:-1], ww, dd, 1.0)
    with pytest.raises(ValueError):
        episode_metrics(r, v, ww[:, :-1], dd, 1.0)
    with pytest.raises(ValueError):
        episode_metrics(r, v, ww, dd[:-1], 1.0)
    with pytest.raises(ValueError):
        episode_metrics(r, v, ww, dd, 1.0, max_episodes=0)
    auto = episode_metrics(r, v, ww, dd, 1.0)                    # K = the most dones + 1: holds every episode
    assert auto["sharpe"].shape[1] == int((d != 0).sum(0).max()) + 1 >= int(auto["count"].max())
    as_bool = episode_metrics(r, v, ww, dd.bool(), 1.0)
    assert all(torch.equal(auto[k].view(torch.int64) if auto[k].dtype == torch.float64 else auto[k],
                           as_bool[k].view(torch.int64) if auto[k].dtype == torch.float64 else as_bool[k])
               for k in auto)


# ------------------------------------------------------------------ the Python layers
EB, EN, EW, EF, ESTEPS = 70, 5, 6, 5, 24


def _setup(seed=3):
    from pmenv import Episodes, MarketSeries, TradingEnv, synth
    days = 64
    ms = MarketSeries(synth.series(days, 1, EN, seed=17, device=DEV)[:, 0].contiguous(), device=DEV)
    rng = np.random.default_rng(seed)
    start = rng.integers(0, EW + 1, EB)
    restart = rng.integers(0, 20, EB)
    length = 3 + np.arange(EB) % 7                               # per-env lengths 3 .. 9
    env = TradingEnv(num_envs=EB, num_assets=EN, window=EW, features=EF, device=DEV, track_info=False)
    ep = Episodes(ms, EW, start, restart=restart, length=length)
    obs = ms.initial_window(ep.start, EW)
    env.reset(obs)
    return ms, env, ep, obs


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def test_gpu_evaluate_matches_a_manual_loop_through_the_restatement():
    from pmenv import episodes, synth
    act = synth.actions(ESTEPS, EB, EN, seed=11, device=DEV)
    ms, env, ep, obs = _setup()
    got = episodes.evaluate(env, ms, ep, obs, ESTEPS, act=act)
    # the record, rebuilt by hand on a second env with the same actions
    ms2, env2, ep2, obs2 = _setup()
    rets = torch.empty(ESTEPS, EB, dtype=torch.float64, device=DEV)
    vals = torch.empty(ESTEPS + 1, EB, dtype=torch.float64, device=DEV)
    wts = torch.empty(ESTEPS + 1, EB, EN, device=DEV)
    dones = torch.empty(ESTEPS, EB, dtype=torch.uint8, device=DEV)
    rews = torch.empty(ESTEPS, EB, device=DEV)
    vals[0] = env2.value
    wts[0] = 0.0
    wts[0, :, 0] = 1.0                                           # a reset env holds e0
    for t in range(ESTEPS):
        ro, wo = torch.empty(EB, dtype=torch.float64, device=DEV), torch.empty(EB, EN, device=DEV)
        rews[t], _ = env2.step(act[t], obs2, series=ms2, day=ep2.next_day, weights_out=wo, returns_out=ro)
        rets[t], wts[t + 1], vals[t + 1] = ro - 1.0, wo, env2.value.clone()
        dones[t] = env2.restart(obs2, ep2)
    assert float(vals[0, 0]) == env2.cfg.init_cash
    ret_h, val_h, w_h, d_h = (x.cpu().numpy() for x in (rets, vals, wts, dones))
    assert d_h.sum(0).min() >= 2 and len(set(d_h.sum(0).tolist())) > 1
    refs = mr.ref(ret_h, val_h, w_h, d_h, env2.cfg.init_cash, 0.04, 252.0)
    K = int(d_h.sum(0).max()) + 1
    out, span, count = _unpack(got)
    assert out.shape == (EB, K, 5)
    _compare((out, span, count), refs, K, val_h)
    # every closed episode's final value is the terminal value seen before the restart
    closed = 0
    for b in range(EB):
        for k in range(count[b]):
            last = span[b, k, 1]
            if d_h[last - 1, b]:
                closed += 1
                assert out[b, k, 4] == val_h[last, b] and val_h[last, b] != env2.cfg.init_cash
    assert closed >= 2 * EB
    # the additive outputs change nothing: the rewards are episodes.collect's
    ms3, env3, ep3, obs3 = _setup()
    rew3, d3 = episodes.collect(env3, ms3, ep3, obs3, ESTEPS, act=act)
    assert _bits_equal(rew3, rews) and torch.equal(d3, dones.bool())
    assert _bits_equal(obs, obs2) and _bits_equal(obs, obs3) and _bits_equal(env.value, env3.value)


def test_gpu_step_returns_out_is_info_returns():
    from pmenv import MarketSeries, TradingEnv, synth
    ms = MarketSeries(synth.series(40, 1, EN, seed=17, device=DEV)[:, 0].contiguous(), device=DEV)
    act = synth.actions(10, 1, EN, seed=5, device=DEV)
    start = torch.zeros(1, dtype=torch.int32, device=DEV)
    ea = TradingEnv(num_envs=1, num_assets=EN, window=EW, features=EF, device=DEV, track_info=True)
    eb = TradingEnv(num_envs=1, num_assets=EN, window=EW, features=EF, device=DEV, track_info=False)
    oa, ob = ms.initial_window(start, EW), ms.initial_window(start, EW)
    ea.reset(oa)
    eb.reset(ob)
    ro = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    for t in range(10):
        day = start + EW + t
        ra, _ = ea.step(act[t], oa, series=ms, day=day)
        rb, _ = eb.step(act[t], ob, series=ms, day=day, returns_out=ro)
        assert _bits_equal(ra, rb)
        assert _bits_equal(torch.as_tensor(ea.info["returns"][-1]).reshape(1).to(DEV), ro), t
    with pytest.raises(ValueError):
        eb.step(act[0], ob, series=ms, day=start + EW + 10, returns_out=ro.float())
    # an env that keeps info records the same ratio when the caller also asks for it
    rc = torch.empty(1, dtype=torch.float64, device=DEV)
    ea.step(act[0], oa, series=ms, day=start + EW + 10, returns_out=rc)
    assert _bits_equal(torch.as_tensor(ea.info["returns"][-1]).reshape(1).to(DEV), rc)


def test_gpu_off_policy_evaluate_episodes_is_episodes_evaluate():
    from pmenv import episodes, synth
    from pmenv.off_policy import OffPolicy
    act = synth.actions(ESTEPS, EB, EN, seed=11, device=DEV)
    ms, env, ep, obs = _setup()
    want = episodes.evaluate(env, ms, ep, obs, ESTEPS, act=act, max_episodes=9)
    ms2, env2, ep2, obs2 = _setup()
    loop = OffPolicy(env2, ms2, capacity=32, episodes=True)
    got = loop.evaluate_episodes(ep2, obs2, ESTEPS, act=act, max_episodes=9)
    assert set(got) == set(want) == set(KEYS) | {"first", "last", "count"}
    for k in want:
        assert _bits_equal(got[k], want[k]), k
    assert loop.replay.count == 0                                # an evaluation records nothing
