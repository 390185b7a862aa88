"""Per-env episodes on a resident market series.

Every other driver of this package is lockstep: all B envs reset at once, so a batch of envs
at random start days is cut to what the latest-starting env has left of the series. The
reference's own episode is "walk the training series to its end" (`train/on_policy.py:59-67`):
envs that start on different days end on different steps, and batched envs elsewhere
(gymnasium's VectorEnv, EnvPool, Isaac Gym) restart each env by itself when its episode ends.

`Episodes` keeps the per-env day counters on the device and `TradingEnv.restart(features,
episodes)` is one `pmenv_restart_days` launch after every `step(series=, day=)`: the envs
whose episode ended get their restart day's window and the reset state, the others only a
day counter one higher; the launch's work is proportional to the envs that restart.

The day convention is the second of the two the design offered, `episodes.next_day`:

    r, _ = env.step(a, obs, series=series, day=episodes.next_day)
    done = env.restart(obs, episodes)

`next_day[b]` is the bar env b's next step appends — the value `step(day=...)` takes, the same
"bar each env appends next" OffPolicy.collect counts — and it is the array the kernel
updates: when the restart call runs, `next_day[b]` is the bar the step just appended; after
it, `next_day[b] + 1`, or `restart[b] + window` for an env that restarted. `episodes.day` is
`next_day - 1`, the latest bar in each env's window: `start + window - 1` at first, so the
first step's day is `day + 1 = start + window`.
"""
import numpy as np
import torch

from .config import RISK_FREE_RATE


def _days_of(series):
    if hasattr(series, "days"):
        return int(series.days)
    if torch.is_tensor(series):
        return int(series.shape[0])
    return int(series)


class Episodes:
    def __init__(self, series, window, start, end=None, restart=None, length=None, device=None):
        """series: the MarketSeries (or [T, N, F-1] tensor) the steps read; a plain day count
        serves host-side bookkeeping (device="cpu"), which needs no series.
        start [B]: first day of each env's initial window. end [B]: one past the last bar env
        b may append (None: the series' end for every env, the reference's episode).
        restart [B]: first day of the window an env restarts on (None: start).
        length (int or [B]): bars per episode — end starts as start + window + length, and
        after every restart() the envs that restarted get end = restart + window + length
        (torch ops on the device, no sync); end= and length= exclude each other.
        Raises ValueError naming the first env whose days do not fit the series."""
        days = _days_of(series)
        W = int(window)
        bars = getattr(series, "bars", series if torch.is_tensor(series) else None)
        if device is None:
            device = bars.device if bars is not None else "cuda"
        self.device = torch.device(device)
        self.bars = bars
        self.days, self.window = days, W

        def host(x, name):
            a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
            a = a.astype(np.int64).reshape(-1)
            if a.size == 1 and name != "start":
                a = np.broadcast_to(a, (B,))
            if a.size != B:
                raise ValueError(f"{name} must hold one value per env ({B}), got {a.size}")
            return a

        B = int(np.asarray(start.detach().cpu() if torch.is_tensor(start) else start).size)
        if B < 1:
            raise ValueError("start must hold one day per env")
        st = host(start, "start")
        rs = st if restart is None else host(restart, "restart")
        if end is not None and length is not None:
            raise ValueError("end= and length= exclude each other")
        ln = None
        if length is not None:
            ln = host(length, "length")
            en = st + W + ln
        else:
            en = np.full(B, days, np.int64) if end is None else host(end, "end")

        def first_bad(bad, what):
            if bad.any():
                b = int(np.argmax(bad))
                raise ValueError(f"env {b}: {what} (start {st[b]}, restart {rs[b]}, end {en[b]}, window {W}, "
                                 f"series of {days} days)")

        if ln is not None:
            first_bad(ln < 1, "length must be at least 1")
        first_bad(st < 0, "start must be >= 0")
        first_bad((rs < 0) | (rs > days - W), "restart must be in [0, days - window]")
        first_bad(en > days, "end must be <= the series' days")
        if ln is None:
            first_bad(rs + W >= en, "restart + window must be < end")
        else:       # the end in force after a restart is restart + window + length (> restart + window)
            first_bad(rs + W + ln > days, "restart + window + length must be <= the series' days")
        first_bad(st + W >= en, "start + window must be < end")

        def up(a):
            return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=self.device)

        self.num_envs = B
        self.start = up(st)
        self.next_day = up(st + W)          # the kernel's `day` array: the bar the next step appends
        self.end = up(en)
        self.restart = up(rs)
        self.done = torch.zeros(B, dtype=torch.uint8, device=self.device)
        self._end_restart = up(rs + W + ln) if ln is not None else None

    @property
    def day(self):
        """The latest bar in each env's window (next_day - 1)."""
        return self.next_day - 1

    def _restarted(self):
        """After a restart call wrote `done`: episodes of fixed length end `length` bars after
        the window they restarted on."""
        if self._end_restart is not None:
            self.end.copy_(torch.where(self.done.bool(), self._end_restart, self.end))

    def advance_host(self):
        """The day bookkeeping of one restart call for host tensors (device="cpu"): planning and
        tests without a GPU. It moves no window and no env state — on the GPU that is
        TradingEnv.restart, one kernel."""
        if self.device.type != "cpu":
            raise ValueError("advance_host is the host-side bookkeeping; on the GPU call TradingEnv.restart")
        nxt = self.next_day + 1
        done = nxt >= self.end
        self.next_day.copy_(torch.where(done, self.restart + self.window, nxt))
        self.done.copy_(done.to(torch.uint8))
        self._restarted()
        return self.done


def collect(env, series, episodes, obs, steps, act=None):
    """The continuous loop act -> env.step(series=, day=) -> env.restart for `steps` steps.
    obs: the envs' windows (series.initial_window(episodes.start, W), reset), advanced in
    place. act: None (uniform weights), a [steps, B, N] tensor, or a callable obs -> [B, N].
    Returns (rewards [steps, B] f32, dones [steps, B] bool): dones[t, b] says env b's episode
    ended with step t, the layout rollout.gae takes."""
    B, N = env.cfg.num_envs, env.cfg.num_assets
    rewards = torch.empty(steps, B, dtype=torch.float32, device=env.device)
    dones = torch.empty(steps, B, dtype=torch.uint8, device=env.device)
    uniform = torch.full((B, N), 1.0 / N, device=env.device) if act is None else None
    for t in range(steps):
        if uniform is not None:
            a = uniform
        elif callable(act):
            with torch.no_grad():
                a = act(obs)
        else:
            a = act[t]
        r, _ = env.step(a, obs, series=series, day=episodes.next_day)
        rewards[t] = r
        dones[t] = env.restart(obs, episodes)
    return rewards, dones.bool()


def evaluate(env, series, episodes, obs, steps, act=None, max_episodes=None, risk_free_rate=RISK_FREE_RATE,
             periods=252):
    """The `collect` loop as an evaluation run: per-episode Sharpe, Sortino, max drawdown,
    average turnover and final value for envs that end their episodes on different steps
    (the reference's Metrics are per episode: walk the series to its end, then metrics.write(),
    train/off_policy.py:96-110). Per step it records the return (step(returns_out=) - 1), a
    copy of env.value taken between step and restart — the terminal value where the step ended
    an episode —, the step's post-drift weights and the done restart returns; row 0 holds the
    envs' value and last post-drift weights at entry. Returns replay.episode_metrics(...) of
    that record with init_value = env.cfg.init_cash; an env that is not freshly reset at entry
    has its first episode measured from its entry value. max_episodes=None costs one host
    read after the run."""
    from .replay import episode_metrics
    B, N = env.cfg.num_envs, env.cfg.num_assets
    dev = env.device
    rets = torch.empty(steps, B, dtype=torch.float64, device=dev)
    vals = torch.empty(steps + 1, B, dtype=torch.float64, device=dev)
    wts = torch.empty(steps + 1, B, N, dtype=torch.float32, device=dev)
    dones = torch.empty(steps, B, dtype=torch.uint8, device=dev)
    vals[0] = env.value
    wts[0] = env.weights.get_last()
    uniform = torch.full((B, N), 1.0 / N, device=dev) if act is None else None
    for t in range(steps):
        if uniform is not None:
            a = uniform
        elif callable(act):
            with torch.no_grad():
                a = act(obs)
        else:
            a = act[t]
        env.step(a, obs, series=series, day=episodes.next_day, weights_out=wts[t + 1], returns_out=rets[t])
        vals[t + 1] = env.value                   # before the restart puts init_cash back
        dones[t] = env.restart(obs, episodes)
    rets -= 1.0
    return episode_metrics(rets, vals, wts, dones, env.cfg.init_cash, max_episodes, risk_free_rate, periods)
