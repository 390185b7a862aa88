"""An off-policy training loop over B lockstep envs — the shape of train/off_policy.py
(`Train._collect_rand` :60-71, `_collect` :73-86, `_update_off_policy` :88-94,
`_evaluate_off_policy` :96-110) with the market data, the env step, the replay buffer
and the evaluation metrics all on device.

    reference (one env)                          here (B envs)
    self.s = env.reset(feat)             :65     obs = series.initial_window(start, W); env.reset(obs)
    a = agent.act(s, is_random=True)     :67     a = random simplex weights           (collect_rand)
    a = agent.act(s)                     :81     a = act(obs)                          (torch, no grad)
    r, s_ = env.step(a, feat, targ)      :68     env.step(a, obs, series=series, day=day)   in place
    buffer.add(epoch, step, a, r)        :69     replay.add(day - 1, a, r)             (DeviceReplay)
    s, a, r, s_ = buffer.sample()        :91     replay.sample(batch_size)             (HIP gather)
    agent.update(epoch, step, s, a, r, s_) :92   update(s, a, r, s_)                   (caller's agent)
    add_experience's n_step fold (td3.py:85-106) replay.sample_nstep(batch_size, n)    (n_step > 1: HIP gather,
                                                 update(s, a, R, s_, discount)          folded at sample time)
    x, a, r = data["x"], data["a"], data["r"]    replay.sample_sequences(batch_size, L) (seq_len > 0: HIP gather,
      (agent/dreamer/dreamer.py:78)              update(x, a, r)                        [L, S, ..] time-major)
    samples, idxs, weights = replay_buffer.sample(..) replay.sample_prioritized(batch_size)  (prioritized: HIP sum tree,
    update_priorities(idxs, td_error)            td = update(s, a, r, s_, weights);     agent/td3/td3.py:118-144)
      (agent/td3/td3.py:118,144)                 replay.update_priorities(leaf, td)
    metrics.write()                      :110    trajectory_metrics(...)               (HIP reductions)
    (one env walks the series to its end, :60-86)  collect_episodes(ep, obs, steps)      (episodes=True: every env ends
                                                 replay.add(d, a, r, done=done)         and restarts on its own)

Every env trades the one HBM-resident series (pmenv.data.MarketSeries) from its own
start day: the step reads day[b]'s bar straight from the series (no per-step host
feed). The agent (DSAC / TD3 / DreamerV3 in the reference) is out of scope: `act`
and `update` are the caller's callables.
"""
import torch

from . import episodes as _episodes
from .replay import DeviceReplay, trajectory_metrics


class OffPolicy:
    def __init__(self, env, series, capacity, act=None, update=None, batch_size=256, generator=None,
                 n_step=1, gamma=0.997, seq_len=0, prioritized=False, alpha=0.6, beta=0.4, beta_increment=0.0,
                 episodes=False):
        """env: a pmenv.TradingEnv over B envs; series: pmenv.data.MarketSeries [T, N, F-1];
        capacity: replay steps kept per env (buffer.py's ring); act(obs [B, N, W, F]) ->
        [B, N] weights; update(s, a, r, s_) -> anything (one agent update). n_step > 1
        (agent/td3/td3.py:85-106; gamma: config/dsac.py:30): update(s, a, R, s_, discount)
        with R the discounted sum of up to n_step rewards, s_ the state after the last of
        them and discount [S] = gamma ** (rewards folded), the factor of the bootstrap term.
        seq_len > 0 (agent/dreamer/dreamer.py:77-80; config/dreamer.py:5 BATCH_LEN):
        update(x, a, r) with one batch of batch_size full-length sequences, time-major:
        x [seq_len, S, N, W, F], a [seq_len, S, N], r [seq_len, S].
        prioritized (agent/td3/td3.py:39,118-144): batches are drawn by priority and
        update(s, a, r, s_, weights) -> td_error [S] — with n_step > 1 update(s, a, R, s_,
        discount, weights) — whose result goes to replay.update_priorities; weights [S] are
        the importance weights of the critic loss (:126,143). Not with seq_len > 0.
        episodes: the envs end and restart on their own (`collect_episodes` over a
        pmenv.episodes.Episodes); the replay keeps an episode id per (row, env), so no sample
        of any kind spans an env's restart."""
        if n_step < 1 or not 0.0 < gamma <= 1.0:
            raise ValueError("n_step must be >= 1 and gamma in (0, 1]")
        if seq_len < 0 or (seq_len > 0 and n_step > 1):
            raise ValueError("seq_len must be >= 0, and sequences do not combine with n_step > 1")
        if prioritized and seq_len > 0:
            raise ValueError("sequence samples stay uniform: prioritized does not combine with seq_len > 0")
        cfg = env.cfg
        if series.num_assets != cfg.num_assets or series.channels != cfg.features - 1:
            raise ValueError("series must be [T, num_assets, features - 1]")
        self.env, self.series = env, series
        self.B, self.N, self.W = cfg.num_envs, cfg.num_assets, cfg.window
        self.replay = DeviceReplay(self.B, self.N, self.W, capacity, series, cfg.features, prioritized=prioritized,
                                   alpha=alpha, beta=beta, beta_increment=beta_increment, per_env=episodes)
        self.episodes = bool(episodes)
        self.act_fn, self.update_fn = act, update
        self.batch_size = batch_size
        self.generator = generator
        self.n_step, self.gamma = n_step, gamma
        self.seq_len = seq_len
        self.prioritized = prioritized

    def _random_action(self):
        """agent.act(s, is_random=True): uniform random portfolio weights (a simplex point)."""
        g = torch.empty(self.B, self.N, device=self.env.device).exponential_()
        return g / g.sum(-1, keepdim=True)

    def collect(self, start, steps, random=False):
        """_collect_rand / _collect (off_policy.py:60-86) for every env: reset on the window
        ending the day before start + W, then `steps` steps, each recorded in the replay.
        start: [B] first day of each env's initial window. Returns (rewards [steps, B], obs)."""
        start = torch.as_tensor(start, device=self.env.device).to(torch.int32).reshape(self.B)
        if int(start.max()) + self.W + steps > self.series.days:
            raise ValueError("series too short for start + window + steps")
        obs = self.series.initial_window(start, self.W)
        self.env.reset(obs)
        self.replay.new_episode()                 # no sampled window spans the reset
        day = start + self.W                      # the bar each env appends next
        rewards = []
        for _ in range(steps):
            if random or self.act_fn is None:
                a = self._random_action()
            else:
                with torch.no_grad():
                    a = self.act_fn(obs)
            r, _ = self.env.step(a, obs, series=self.series, day=day)
            self.replay.add(day - 1, a, r)        # the day of the window the action was taken on
            rewards.append(r)
            day = day + 1
        return torch.stack(rewards), obs

    def collect_episodes(self, ep, obs, steps, random=False):
        """The continuous loop of pmenv.episodes.collect with every step recorded: act ->
        env.step(series=, day=ep.next_day) -> env.restart -> replay.add(.., done=). ep: the
        Episodes of the envs; obs: their windows (series.initial_window(ep.start, W), reset),
        advanced in place. Returns (rewards [steps, B] f32, dones [steps, B] bool)."""
        if not self.episodes:
            raise ValueError("collect_episodes needs OffPolicy(episodes=True)")
        rewards = torch.empty(steps, self.B, dtype=torch.float32, device=self.env.device)
        dones = torch.empty(steps, self.B, dtype=torch.uint8, device=self.env.device)
        for t in range(steps):
            if random or self.act_fn is None:
                a = self._random_action()
            else:
                with torch.no_grad():
                    a = self.act_fn(obs)
            d = ep.next_day - 1                   # the day of the window the action is taken on
            r, _ = self.env.step(a, obs, series=self.series, day=ep.next_day)
            done = self.env.restart(obs, ep)      # rewrites next_day
            self.replay.add(d, a, r, done=done)
            rewards[t] = r
            dones[t] = done
        return rewards, dones.bool()

    def update(self, steps):
        """_update_off_policy (off_policy.py:88-94): `steps` sampled batches into update()."""
        out = []
        for _ in range(steps):
            if self.seq_len > 0:
                x, a, r, _ = self.replay.sample_sequences(self.batch_size, self.seq_len, self.generator)
                out.append(self.update_fn(x, a, r) if self.update_fn is not None else None)
                continue
            if self.prioritized:
                if self.n_step > 1:
                    s, a, r, s_, _, disc, leaf, w = self.replay.sample_nstep_prioritized(
                        self.batch_size, self.n_step, self.gamma, self.generator)
                    args = (s, a, r, s_, disc, w)
                else:
                    s, a, r, s_, leaf, w = self.replay.sample_prioritized(self.batch_size, self.generator)
                    args = (s, a, r, s_, w)
                td = self.update_fn(*args) if self.update_fn is not None else None
                if td is not None:
                    self.replay.update_priorities(leaf, td)
                out.append(td)
                continue
            if self.n_step > 1:
                s, a, r, s_, _, disc = self.replay.sample_nstep(self.batch_size, self.n_step, self.gamma,
                                                                self.generator)
                out.append(self.update_fn(s, a, r, s_, disc) if self.update_fn is not None else None)
                continue
            s, a, r, s_ = self.replay.sample(self.batch_size, self.generator)
            out.append(self.update_fn(s, a, r, s_) if self.update_fn is not None else None)
        return out

    def evaluate(self, start, steps, act=None):
        """_evaluate_off_policy (off_policy.py:96-110) + Metrics (util/eval.py:14-37): a
        deterministic run of `steps` days from `start`, then per-env Sharpe, Sortino,
        max drawdown, average turnover and final value ({name: [B] f64})."""
        act = act or self.act_fn
        env = self.env
        track = env.track_info
        env.track_info = True
        try:
            start = torch.as_tensor(start, device=env.device).to(torch.int32).reshape(self.B)
            obs = self.series.initial_window(start, self.W)
            env.reset(obs)
            day = start + self.W
            for _ in range(steps):
                with torch.no_grad():
                    a = act(obs) if act is not None else self._random_action()
                env.step(a, obs, series=self.series, day=day)
                day = day + 1
            rets = torch.stack(env.info["returns"][1:]) - 1.0          # [T, B] simple returns
            vals = torch.stack(env.info["values"])                     # [T+1, B]
            wts = torch.stack(env.info["actions"])                     # [T+1, B, N] post-drift weights
            return trajectory_metrics(rets, vals, wts)
        finally:
            env.track_info = track

    def evaluate_episodes(self, ep, obs, steps, act=None, **kw):
        """`evaluate` for envs that end their episodes on their own: pmenv.episodes.evaluate
        over this loop's env and series — per-episode metrics, {name: [B, K]} with first /
        last / count — with `act` (default: the loop's act; None: uniform weights). Records
        nothing in the replay. kw: max_episodes, risk_free_rate, periods."""
        return _episodes.evaluate(self.env, self.series, ep, obs, steps,
                                  act if act is not None else self.act_fn, **kw)
