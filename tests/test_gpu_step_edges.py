"""Every scalar-step form on heterogeneous edge-case batches (tests/edge_inputs.py), against
the CPU restatement at test_gpu_parity._run_both's tolerances, unchanged: reward 1e-6 |r| +
1e-9, return and value rtol 1e-12, w', ring and weight channel rtol 2e-7 / atol 1e-12, market
channels bit-equal, counters equal (test_step_edges_host.py pins the input preconditions
that make them applicable). Up to 8 envs share a wave in these forms, and their wave-level
shortcuts (__any(not_close), __any(norm), while (__any(!done)), ballots masked per group,
the flat step's owner workgroup) are only exercised when neighbouring envs disagree: here
env b takes action class (b + t) % 10, masked resets stagger the counters, and poison events
hit envs whose neighbours stay healthy. Needs an MI355X.

Legs: finite (all shapes x configs), same bits across paths (include/pmenv.h), non-finite
(element classes, finite elements at the tolerances, the exact non-finite count), host I/O.
"""
import functools

import numpy as np
import pytest
import torch

import edge_inputs as ei

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


def _t(x, dtype=torch.float32, host=False):
    # a copy: the cached batches are shared and read-only, host windows are written in place
    return torch.as_tensor(np.array(x, order="C"), dtype=dtype, device="cpu" if host else DEV)


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _classes(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def _same(got, ref, rtol, atol, what):
    """Element classes (finite, NaN, +inf, -inf) equal; finite elements within atol + rtol |ref|."""
    got, ref = np.asarray(_np(got), np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    cg, cr = _classes(got), _classes(ref)
    if not np.array_equal(cg, cr):
        i = np.argwhere(cg != cr)[0]
        raise AssertionError(f"{what}: class {cg[tuple(i)]} vs the restatement's {cr[tuple(i)]} at {tuple(i)} "
                             f"({np.count_nonzero(cg != cr)} elements)")
    f = cr == 0
    err = np.abs(got[f] - ref[f]) - (atol + rtol * np.abs(ref[f]))
    if err.size and err.max() > 0:
        i = np.argwhere(f)[np.argmax(err)]
        raise AssertionError(f"{what}: {got[tuple(i)]!r} vs {ref[tuple(i)]!r} at {tuple(i)}")


@functools.lru_cache(maxsize=2)
def _reference(shape_id, cfg_id, events, resident):
    """The restatement's run of a case, computed once and shared by its in-place, obs_out and
    per-path tests."""
    shape = _shape(shape_id)
    _, _, mode, N, W, F, B, _ = shape
    cfg = ei.env_config(shape, _config(cfg_id))
    T = ei.steps(W)
    bt = ei.batch(B, N, W, T, F)
    if events:
        bt = ei.poisoned(bt, events, advance=mode == "advance")
    if resident:
        bt = _resident(bt, cfg)
    return cfg, bt, ei.oracle_run(cfg, bt, mode, ei.reset_masks(B, W))


def _shape(shape_id):
    return ei.SHAPE_BY_ID.get(shape_id) or {s[0]: s for s in ei.HOST_SHAPES}[shape_id]


# the Sharpe forms carry the poison in their running statistics until the masked reset clears them
NONFINITE_CONFIGS = {"nf-and": {}, "nf-or": dict(norm="or"), "nf-and-c": dict(commission=0.0025),
                     "nf-or-c": dict(norm="or", commission=0.0025), "nf-sharpe": dict(reward="sharpe_ratio"),
                     "nf-dsharpe-or-c": dict(norm="or", commission=0.0025, reward="diff_sharpe")}


def _config(cfg_id):
    for table in (ei.CONFIGS, ei.FORM_CONFIGS, NONFINITE_CONFIGS):
        if cfg_id in table:
            return table[cfg_id]
    raise KeyError(cfg_id)


def _resident(bt, cfg):
    """The resident-series form of a batch: one market (env 0's series) shared by every env,
    env b starting b % 3 days in, day[t, b] the index of step t's bar; BAD_DAY's env gets a day
    outside [0, series_days) at its step, which reads a NaN bar (include/pmenv.h)."""
    T, B, W = bt["act"].shape[0], cfg.num_envs, cfg.window
    market = np.ascontiguousarray(bt["ser"][:, 0])                    # [W + T, N, Fm]
    market = np.concatenate([market, market[-2:]])                     # the latest starts' last days
    start = np.arange(B) % 3
    day = start[None, :] + W + np.arange(T)[:, None]                   # [T, B]
    bars = market[day]                                                 # [T, B, N, Fm]
    obs0 = np.zeros_like(bt["obs0"])
    for b in range(B):
        obs0[b, :, :, :-1] = market[start[b]:start[b] + W].transpose(1, 0, 2)
    t_bad, b_bad = ei.BAD_DAY
    day = day.copy()
    day[t_bad, b_bad] = market.shape[0] + 7
    bars = bars.copy()
    bars[t_bad, b_bad] = np.nan
    return dict(bt, obs0=obs0, bars=bars, day=day.astype(np.int32), market=market)


def _check_path(env, shape, db):
    """The step path names the kernel this shape is here for, in the window mode driven."""
    _, impl, mode, N, W, F, B, kernel = shape
    if kernel is None:
        return
    path = env.step_path
    part = path.split(" | ")[0 if db else 1] if " | " in path else path
    name = part.split(" (")[0]
    if kernel.startswith("scalar_step"):
        assert name.startswith(kernel + "+"), path           # two launches: scalar kernel + stream
    elif kernel == "advance_gen_kernel":
        assert name == "scalar_step_vec_kernel+advance_gen_kernel", path
    else:
        assert name == kernel, path


def _drive(shape_id, cfg_id, db=False, events=(), host=False, resident=False, every_step_state=False):
    """pmenv.TradingEnv beside the restatement's recorded run, as test_gpu_parity._run_both."""
    from pmenv import TradingEnv, MarketSeries
    shape = _shape(shape_id)
    _, impl, mode, N, W, F, B, _ = shape
    cfg, bt, ref = _reference(shape_id, cfg_id, tuple(events), resident)
    Fm = F - 1
    T = ei.steps(W)
    resets = ei.reset_masks(B, W)
    env = TradingEnv(config=cfg, device=DEV, track_info=True, step_impl=impl)
    _check_path(env, shape, db)
    series = MarketSeries(bt["market"], device=DEV) if resident else None
    obs = _t(bt["obs0"], host=host)
    env.reset(obs)
    for t in range(T):
        if t in resets:
            env.reset(obs, mask=_t(resets[t], torch.bool, host=host))
        a = _t(bt["act"][t], host=host)
        if mode == "surface":
            obs.copy_(_t(ei.surface_window(bt, t, W), host=host))
            r, got = env.step(a, obs, prices=_t(bt["y"][t], host=host))
            assert got is obs
        else:
            kw = dict(series=series, day=_t(bt["day"][t], torch.int32)) if resident else \
                dict(bar=_t(bt["ser"][W + t], host=host))
            if db:
                nxt = torch.full_like(obs, float("nan"))
                prev = obs.clone()
                r, got = env.step(a, obs, out=nxt, **kw)
                assert got is nxt and torch.equal(obs.view(torch.int32), prev.view(torch.int32))   # input untouched
                obs = nxt
            else:
                r, got = env.step(a, obs, **kw)
                assert got is obs
        at = f"step {t}"
        _same(r, ref["r"][t], 1e-6, 1e-9, f"{at}: reward")
        _same(env.info["returns"][-1], ref["ret"][t], 1e-12, 0.0, f"{at}: return")
        _same(env.value, ref["value"][t], 1e-12, 0.0, f"{at}: value")
        _same(env.info["actions"][-1], ref["w"][t], 2e-7, 1e-12, f"{at}: w'")
        go = _np(obs)
        assert np.array_equal(go[..., :Fm], ref["obs"][t][..., :Fm], equal_nan=True), f"{at}: market channels differ"
        _same(go[..., Fm], ref["obs"][t][..., Fm], 2e-7, 1e-12, f"{at}: weight channel")
        if every_step_state or t == T - 1:
            _state(env, ref, t, at)
    assert env.nonfinite_count() == ei.nonfinite_steps(ref), "non-finite (env, step) pairs: doubled or dropped"
    return env


def _state(env, ref, t, at):
    assert np.array_equal(env._counter.cpu().numpy(), ref["k"][t]), f"{at}: counters"
    _same(env._ring, ref["ring"][t], 2e-7, 1e-12, f"{at}: ring")
    # the statistics are running sums of the return (rtol 1e-12): _run_both's bound on stat_a
    _same(env._stat_a, ref["sa"][t], 1e-9, 1e-14, f"{at}: stat_a")
    _same(env._stat_b, ref["sb"][t], 1e-9, 1e-14, f"{at}: stat_b")


# ---------------------------------------------------------------- finite leg
def _finite_params():
    out = []
    for shape, cid, _ in ei.finite_cases():
        if shape in ei.HOST_SHAPES:
            continue
        for db in ((False, True) if shape[2] == "advance" else (False,)):
            out.append(pytest.param(shape[0], cid, db, id=f"{shape[0]}-{cid}-{'obs_out' if db else 'inplace'}"))
    return out


@pytest.mark.parametrize("shape_id,cfg_id,db", _finite_params())
def test_gpu_edge_batch_vs_oracle(shape_id, cfg_id, db):
    """The finite leg: the edge batch through the shape's path and scalar-step form, in place
    and with out=, past the ring's wrap, with two masked resets; the non-finite count is the
    restatement's (0, or the Sharpe ratio's first steps)."""
    _drive(shape_id, cfg_id, db=db)


# ---------------------------------------------------------------- same-bits leg
SAME_BITS_W = {5: 24, 12: 10, 30: 4, 40: 4}       # 150+ chunks per env: the smallest windows the flat step takes


def _record(impl, N, W, kw):
    """The edge batch through one path: every step's reward, value, return, w', ring, counters
    and window."""
    from pmenv import TradingEnv
    from pmenv.config import EnvConfig
    B, T = ei.B_EDGE, ei.steps(W)
    bt = ei.batch(B, N, W, T)
    resets = ei.reset_masks(B, W)
    env = TradingEnv(config=EnvConfig(num_envs=B, num_assets=N, window=W, **kw), device=DEV, track_info=True,
                     step_impl=impl)
    kern = {"two_launch": "+", "one_launch": "step_env_kernel", "relay": "step_relay_kernel",
            "flat": "step_flat_kernel"}[impl]
    assert kern in env.step_path.split(" | ")[1], env.step_path
    obs = _t(bt["obs0"])
    env.reset(obs)
    rec = []
    for t in range(T):
        if t in resets:
            env.reset(obs, mask=_t(resets[t], torch.bool))
        r, _ = env.step(_t(bt["act"][t]), obs, bar=_t(bt["ser"][W + t]))
        rec.append([x.clone() for x in (r, env.value, env.info["returns"][-1], env.info["actions"][-1], env._ring,
                                        env._counter, obs)])
    return rec


_two_launch_record = functools.lru_cache(maxsize=2)(lambda N, W, kw: _record("two_launch", N, W, dict(kw)))
SAME_BITS_CONFIGS = {"reference": (), "c-or": (("commission", 0.0025), ("norm", "or"))}


@pytest.mark.parametrize("cfg_id", list(SAME_BITS_CONFIGS))
@pytest.mark.parametrize("impl,N", [(i, n) for n in SAME_BITS_W for i in ("one_launch", "relay", "flat")] +
                         [("relay", n) for n in (70, 130, 260)])
def test_gpu_edge_batch_same_bits_across_paths(impl, N, cfg_id):
    """include/pmenv.h: for N <= 64 every path gives the same bits, and the relayed step those
    of two launches for every N it takes — on the edge batch, at every step."""
    kw = SAME_BITS_CONFIGS[cfg_id]
    W = SAME_BITS_W.get(N, 4)
    ref = _two_launch_record(N, W, kw)
    got = _record(impl, N, W, dict(kw))
    names = ("reward", "value", "return", "w'", "ring", "counters", "window")
    for t, (g, r) in enumerate(zip(got, ref)):
        for name, x, y in zip(names, g, r):
            assert torch.equal(x, y), f"step {t}: {name} differs from the two-launch step's bits"


# ---------------------------------------------------------------- non-finite leg
@pytest.mark.parametrize("cfg_id", list(NONFINITE_CONFIGS))
@pytest.mark.parametrize("shape_id", ei.NONFINITE_SHAPES)
def test_gpu_edge_batch_poisoned(shape_id, cfg_id):
    """One poison event each on chosen envs (edge_inputs.EVENTS), wave neighbours healthy,
    masked resets reviving all but one later: element classes equal the restatement's
    everywhere (reward, return, value, w', window, ring, statistics, every step), finite
    elements at the usual tolerances — so healthy neighbours and revived envs match as in
    the finite leg — and nonfinite_count() is exactly the restatement's count. No event is
    restricted: every one runs without and with commission."""
    _drive(shape_id, cfg_id, events=ei.EVENTS, every_step_state=True)


ACTION_EVENTS = tuple(e for e in ei.EVENTS if e[2].endswith("_action"))


@pytest.mark.parametrize("cfg_id", ["nf-and", "nf-or-c"])
@pytest.mark.parametrize("shape_id,db", [("two_launch-n30", False), ("two_launch-n70", True), ("one_launch-n30", True),
                                         ("relay-n30", False), ("flat-n30-w4", False), ("tiny-n7-w6-f3", False)])
def test_gpu_edge_batch_poisoned_resident_series(shape_id, cfg_id, db):
    """The resident-series call shape (series=, day=): a day outside [0, series_days) reads
    a NaN bar for that env alone, counted once, beside the action events (the price events
    would poison the one market every env shares)."""
    _drive(shape_id, cfg_id, db=db, events=ACTION_EVENTS, resident=True, every_step_state=True)


# ---------------------------------------------------------------- host-I/O leg
@pytest.mark.parametrize("cfg_id,events", [(c, ()) for c in ei.CONFIGS] +
                         [("nf-and", ei.HOST_EVENTS), ("nf-or-c", ei.HOST_EVENTS)],
                         ids=lambda v: v if isinstance(v, str) else ("poisoned" if v else "finite"))
@pytest.mark.parametrize("shape_id", [s[0] for s in ei.HOST_SHAPES])
def test_gpu_edge_batch_host_io(shape_id, cfg_id, events):
    """The reference driver's call shape with CPU tensors (pmenv_step_host): B = 8 on the
    resident workgroup, B = 9 launched; the finite and the poisoned batch."""
    _drive(shape_id, cfg_id, events=events, host=True, every_step_state=bool(events))
