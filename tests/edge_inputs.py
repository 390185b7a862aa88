"""Adversarial per-env step inputs, and the case tables of the edge tests.

Deterministic generators of heterogeneous batches that both the HIP step and the CPU
restatement (oracle/) consume: neighbouring envs always fall in different action classes
(normalised / left alone, leveraged, one-hot, peaked, just inside / outside isclose), the
price relatives hold a dead asset and a jump, and poison events (non-finite actions and
prices) hit chosen envs whose wave neighbours stay healthy. test_step_edges_host.py pins
the preconditions that make the project's parity tolerances applicable to these inputs;
test_gpu_step_edges.py drives every scalar-step form with them.
"""
import functools

import numpy as np

K = 10                      # action classes; env b at step t takes class (b + t) % K
MIN_ASSETS = 5              # below, classes collide (N - 1, N // 2 and the fixed indices 0 .. 3)
ISCLOSE = 1e-6 + 1e-5       # torch.isclose(sum, 1) defaults: |sum - 1| <= atol + rtol * 1


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def action_row(cls, s, z):
    """One env's action of class `cls` from a simplex sample s = softmax(z), in float64.
                                                              AND mode      OR mode
    0  s                                                      untouched     untouched
    1  s, a[1] -= .3, a[2] += .3  (sum 1, a negative entry)   untouched     softmax
    2  2 s                        (sum 2, non-negative)       leveraged     softmax
    3  z                                                      softmax       softmax
    4  one-hot cash                                           untouched     untouched
    5  one-hot asset N-1                                      untouched     untouched
    6  20 z                       (w' down to denormals)      softmax       softmax
    7  s (1 + 5e-6), a[N-1] -= .2, a[0] += .2 (inside isclose) untouched    softmax
    8  as 7 with 5e-5             (outside isclose)           softmax       softmax
    9  s, a[N // 2] = 0           (sum < 1, non-negative)     untouched     softmax"""
    N = s.shape[0]
    a = s.copy()
    if cls == 1:
        a[1] -= 0.3
        a[2] += 0.3
    elif cls == 2:
        a = 2.0 * s
    elif cls == 3:
        a = z.copy()
    elif cls == 4:
        a[:] = 0.0
        a[0] = 1.0
    elif cls == 5:
        a[:] = 0.0
        a[N - 1] = 1.0
    elif cls == 6:
        a = 20.0 * z
    elif cls in (7, 8):
        a = s * (1.0 + (5e-6 if cls == 7 else 5e-5))
        a[N - 1] -= 0.2
        a[0] += 0.2
    elif cls == 9:
        a[N // 2] = 0.0
    return a


def actions(rng, B, N, t):
    """float32 [B, N]: env b takes class (b + t) % K, so wave neighbours always differ and
    every env visits every class over K steps."""
    assert N >= MIN_ASSETS
    z = rng.standard_normal((B, N))
    s = _softmax(z)
    return np.stack([action_row((b + t) % K, s[b], z[b]) for b in range(B)]).astype(np.float32)


def relatives(rng, B, N, t, series=False):
    """float64 [B, N] price relatives exp(0.02 normal) with a dead asset (y[::7, 3] = 0) and
    a jump (y[3::11, 2] = 30). series=True: the form a close series can carry (a close of 0
    would make every later relative NaN, and 30^T overflows float32): every eighth step the
    dead asset falls by 2^-8 and, four steps off, the jump asset gains 30-fold, neither ever
    reversed (a reversal on a leveraged env cancels most of its value: sum |w'| of 7).
    Every env's day also carries a market move of 3 % or more either way: wide diversified
    portfolios (N = 520) otherwise return so close to 1 that the differential Sharpe ratio's
    variance lands on its 1e-12 switch (test_step_edges_host.py pins that it does not)."""
    m = rng.standard_normal((B, 1))
    y = np.exp(0.02 * rng.standard_normal((B, N)) + np.sign(m) * (0.03 + 0.02 * np.abs(m)))
    if not series:
        y[::7, 3] = 0.0
        y[3::11, 2] = 30.0
    else:
        if t % 8 == 4:
            y[::7, 3] = 2.0 ** -8
        if t % 8 == 0:
            y[3::11, 2] = 30.0
    return y


def isclose_margin(act):
    """min over rows of | |sum - 1| - ISCLOSE | with the float32 entries summed in float64:
    how far the normalisation decision is from flipping under a different summation order."""
    s = act.astype(np.float64).sum(-1)
    return float(np.min(np.abs(np.abs(s - 1.0) - ISCLOSE)))


@functools.lru_cache(maxsize=8)
def batch(B, N, W, T, F=5, close_channel=None, seed=0):
    """One run's inputs: act [T, B, N] f32, y [T, B, N] f32 (the surface contract's prices),
    ser [W + T, B, N, F-1] f32 (a close series whose consecutive ratios are the series-form
    relatives, the other channels beside it) and the first window obs0 [B, N, W, F]."""
    rng = np.random.default_rng([seed, B, N, W, T, F])
    Fm = F - 1
    cc = min(3, Fm - 1) if close_channel is None else close_channel
    act = np.stack([actions(rng, B, N, t) for t in range(T)])
    y = np.stack([relatives(rng, B, N, t) for t in range(T)]).astype(np.float32)
    closes = np.empty((W + T, B, N))
    closes[:W] = 100 * np.exp(np.cumsum(0.01 * rng.standard_normal((W, B, N)), axis=0))
    for t in range(T):
        closes[W + t] = closes[W + t - 1] * relatives(rng, B, N, t, series=True)
    ser = np.empty((W + T, B, N, Fm), np.float32)
    for f in range(Fm):
        ser[..., f] = closes * np.exp(0.002 * rng.standard_normal(closes.shape))
    ser[..., cc] = closes
    obs0 = np.zeros((B, N, W, F), np.float32)
    obs0[..., :Fm] = ser[:W].transpose(1, 2, 0, 3)
    for a in (act, y, ser, obs0):
        a.setflags(write=False)
    return {"act": act, "y": y, "ser": ser, "obs0": obs0, "close_channel": cc}


def reset_masks(B, W):
    """Masked resets at two steps past the ring's fill, so that counters, the ring-full
    state and the Sharpe m < 2 state differ inside a wave."""
    b = np.arange(B)
    return {W + 1: b % 3 == 0, W + 3: b % 5 == 1}


# ---------------------------------------------------------------- poison events
# (step, env, kind): one event each, on envs whose wave neighbours stay healthy (8 envs per
# wave in the densest form). Envs 3, 6, 9, 12 are revived by the first masked reset (b % 3
# == 0), 11 and 16 by the second (b % 5 == 1); env 22 is never reset and stays poisoned.
EVENTS = ((1, 3, "zero_action"), (2, 6, "nan_action"), (3, 9, "big_action"), (2, 11, "nan_price"),
          (4, 12, "inf_price"), (3, 16, "zero_price_held"), (5, 22, "nan_action"))
BAD_DAY = (2, 18)           # (step, env) of the resident-series case's out-of-range day
# the host-I/O leg's batches hold 8 and 9 envs: 0, 3, 6 and 1 are revived, 4 and 7 stay poisoned
HOST_EVENTS = ((1, 3, "zero_action"), (2, 6, "nan_action"), (3, 0, "big_action"), (2, 1, "nan_price"),
               (4, 4, "inf_price"), (3, 7, "zero_price_held"))


def poisoned(bt, events, advance):
    """bt with the events applied (copies): an all-zero action (value 0 in AND mode, uniform
    in OR); one NaN action entry; an action holding 800 and a negative entry (exp overflows
    to NaN in AND mode, the max-shifted softmax gives a finite one-hot in OR); a NaN price;
    +inf on a held asset; 0 on the only held asset. advance: the price events go into the
    series' close (the relative after the event is then poisoned too), else into y."""
    act, y, ser = bt["act"].copy(), bt["y"].copy(), bt["ser"].copy()
    N, W, cc = act.shape[2], bt["obs0"].shape[2], bt["close_channel"]
    rng = np.random.default_rng(99)

    def price(t, b, n, v):
        if advance:
            ser[W + t, b, n, cc] = v
        else:
            y[t, b, n] = v
    for t, b, kind in events:
        s = _softmax(rng.standard_normal(N)).astype(np.float32)
        if kind == "zero_action":
            act[t, b] = 0.0
        elif kind == "nan_action":
            act[t, b] = s
            act[t, b, N // 2] = np.nan
        elif kind == "big_action":
            act[t, b] = s
            act[t, b, 1] = 800.0
            act[t, b, 2] = -0.5
        elif kind == "nan_price":
            act[t, b] = s
            price(t, b, 1, np.nan)
        elif kind == "inf_price":
            act[t, b] = s
            price(t, b, 1, np.inf)
        elif kind == "zero_price_held":
            act[t, b] = 0.0
            act[t, b, N - 1] = 1.0
            price(t, b, N - 1, 0.0)
        else:
            raise ValueError(kind)
    return dict(bt, act=act, y=y, ser=ser)


# ---------------------------------------------------------------- the restatement's run
def oracle_run(cfg, bt, mode, resets):
    """The CPU restatement over bt: per-step lists of the reward, return, w', value, window,
    ring, statistics and counters (copies), as the GPU legs compare them."""
    from oracle import OracleEnv
    T, W = bt["act"].shape[0], cfg.window
    Fm = cfg.features - 1
    env = OracleEnv(cfg)
    obs = bt["obs0"].copy()
    env.reset(obs)
    out = {k: [] for k in ("r", "ret", "w", "value", "obs", "ring", "sa", "sb", "k")}
    for t in range(T):
        if t in resets:
            env.reset(obs, mask=resets[t])
        if mode == "surface":
            obs[...] = surface_window(bt, t, W)
            r, ret, w = env.step(bt["act"][t], obs, prices=bt["y"][t])
        else:
            bar = bt["bars"][t] if "bars" in bt else bt["ser"][W + t]
            r, ret, w = env.step(bt["act"][t], obs, bar=bar)
        for k, v in zip(out, (r, ret, w, env.value, obs, env.ring, env.stat_a, env.stat_b, env.k)):
            out[k].append(np.array(v, copy=True))
    env.close()
    return out


def surface_window(bt, t, W):
    """The caller's next-day window of surface step t (weight channel zero: the step writes it)."""
    win = np.zeros_like(bt["obs0"])
    win[..., :-1] = bt["ser"][t + 1:t + 1 + W].transpose(1, 2, 0, 3)
    return win


def nonfinite_steps(ref):
    """(env, step) pairs whose reward or value is non-finite: what nonfinite_count() counts."""
    return int(sum(np.count_nonzero(~np.isfinite(r) | ~np.isfinite(v)) for r, v in zip(ref["r"], ref["value"])))


# ---------------------------------------------------------------- case tables
B_EDGE = 37                 # ragged last waves at 1, 2, 4 and 8 envs per wave

CONFIGS = {
    "reference": {},
    "or": dict(norm="or"),
    "c25": dict(commission=0.25),
    "c25-or-cap3": dict(commission=0.25, norm="or", mu_max_iter=3),
    "c05-tol-sharpe": dict(commission=0.05, mu_tol=1e-3, reward="sharpe_ratio"),
    "dsharpe-chrono": dict(commission=0.0025, reward="diff_sharpe", ring="chrono"),
}
# on one shape per scalar form
FORM_CONFIGS = {
    "cap0": dict(commission=0.25, mu_max_iter=0),       # the loop skipped: V = (1 - c)^2 V
    "cap1": dict(commission=0.25, mu_max_iter=1),
    "c1e-11": dict(commission=1e-11),                   # done before the first iteration
}

# (id, impl, mode, N, W, F, B, kernel): the smallest shapes that select each scalar-step form.
# kernel: what the step path of that window mode must name (two launches: the scalar kernel).
_TWO = {5: "scalar_step_vec_kernel", 12: "scalar_step_vec_kernel", 30: "scalar_step_reg_kernel",
        40: "scalar_step_reg_kernel", 70: "scalar_step_vec_kernel", 130: "scalar_step_vec_kernel",
        260: "scalar_step_vec_kernel", 520: "scalar_step_kernel"}
# two launches: L8, L16, reg32, reg64, 64x2, 64x4, 64x8 and the LDS form
FORM_SHAPES = [(f"two_launch-n{n}", "two_launch", "advance", n, 4, 5, B_EDGE, k) for n, k in _TWO.items()]
SHAPES = FORM_SHAPES + [
    *[(f"relay-n{n}", "relay", "advance", n, 4, 5, B_EDGE, "step_relay_kernel") for n in (5, 12, 30, 40, 70, 130, 260)],
    *[(f"one_launch-n{n}", "one_launch", "advance", n, 4, 5, B_EDGE, "step_env_kernel") for n in (5, 30, 40)],
    # both 150 chunks per env: tiles straddle envs
    ("flat-n5-w24", "flat", "advance", 5, 24, 5, B_EDGE, "step_flat_kernel"),
    ("flat-n30-w4", "flat", "advance", 30, 4, 5, B_EDGE, "step_flat_kernel"),
    *[(f"flat-n{n}-w16", "flat", "advance", n, 16, 5, B_EDGE, "step_flat_vec_kernel") for n in (70, 130, 260)],
    ("tiny-n7-w6-f3", "auto", "advance", 7, 6, 3, B_EDGE, "step_tiny_kernel"),
    ("small-n30-w20-f4", "auto", "advance", 30, 20, 4, B_EDGE, "step_small_kernel"),     # register form
    ("small-n70-w5-f3", "auto", "advance", 70, 5, 3, B_EDGE, "step_small_kernel"),       # LDS form
    ("lds-n30-w50-f12", "auto", "advance", 30, 50, 12, 5, "step_advance_lds_kernel"),
    ("gen-n6-w4-f8", "two_launch", "advance", 6, 4, 8, B_EDGE, "advance_gen_kernel"),
    ("surface-n9-w8", "auto", "surface", 9, 8, 5, B_EDGE, None),     # surface_body picks the form by N alone
    ("surface-n70-w8", "auto", "surface", 70, 8, 5, B_EDGE, None),
]
SHAPE_BY_ID = {s[0]: s for s in SHAPES}
# the non-finite leg: one shape per scalar form (and per owner / snapshot / relay-word form)
NONFINITE_SHAPES = [s[0] for s in FORM_SHAPES] + ["relay-n30", "relay-n70", "one_launch-n30", "flat-n30-w4", "flat-n70-w16",
                                                  "tiny-n7-w6-f3", "small-n30-w20-f4", "small-n70-w5-f3",
                                                  "surface-n9-w8", "surface-n70-w8"]
# the host-I/O leg: B = 8 the resident workgroup, B = 9 the launched form
HOST_SHAPES = [("host-b8", "auto", "surface", 9, 8, 5, 8, None), ("host-b9", "auto", "surface", 9, 8, 5, 9, None)]


def steps(W):
    return 2 * W + 4        # past the ring's wrap


def env_config(shape, kw):
    """EnvConfig of a shape tuple and config keywords (F < 5: the last market channel closes)."""
    from pmenv.config import EnvConfig
    _, _, _, N, W, F, B, _ = shape
    kw = dict(kw, **({} if F >= 5 else {"close_channel": F - 2}))
    return EnvConfig(num_envs=B, num_assets=N, window=W, features=F, **kw)


def finite_cases():
    """(shape, config id, config keywords) of the finite leg."""
    out = [(s, cid, kw) for s in SHAPES + HOST_SHAPES for cid, kw in CONFIGS.items()]
    out += [(s, cid, kw) for s in FORM_SHAPES for cid, kw in FORM_CONFIGS.items()]
    return out
