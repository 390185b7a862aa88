"""Device replay for vectorised envs.

`DeviceReplay` mirrors replay/buffer.py (`ReplayBuffer.add` :23-37, `.sample` :39-79):
per recorded step it keeps only the day index of the window the agent acted on,
the action and the reward; `sample` re-materialises the observation windows s, s'
on device from the resident market series (pmenv.data.MarketSeries) with the last W
actions as the weight channel, exactly as the reference rebuilds them from its
dataset. `sample_nstep` folds n-step returns at sample time (agent/td3/td3.py:85-106) and
`sample_sequences` serves sequences of consecutive steps (agent/dreamer/dreamer.py:77-80).
`prioritized=True` keeps a resident sum tree over the one-step starts (td3.py:39,118,144;
Schaul et al. 2016, proportional variant): `sample_prioritized`, `update_priorities`.
`per_env=True` keeps an episode id per (ring row, env) on the device, for envs that restart on
their own (`TradingEnv.restart`): every sampling kind then draws from the valid (start, env)
pairs of `valid_pairs`, built and drawn from on the device (csrc/replay_valid.h).
`trajectory_metrics` restates util/eval.py:14-37 (Sharpe, Sortino, max
drawdown, average turnover) per env on device.
"""
import ctypes

import numpy as np
import torch

from . import _abi
from .config import RISK_FREE_RATE


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def valid_starts(row_episode, oldest, count, W, H):
    """Offsets st (from the oldest recorded row) whose W+1 rows st .. st+W all belong to
    one episode — the reference samples a window inside one epoch of its [epoch, step]
    layout (buffer.py:17-21, :47-51). Episode ids only grow along the ring, so the
    first and the last row of a window decide. st < count - W - 1, as buffer.py:50
    draws starts below epoch_len - WINDOW_SIZE - 1. Returns a range when every start is
    valid (the oldest and the newest row share one episode: no scan), else an int64 array."""
    span = max(count - W - 1, 0)
    ep = np.asarray(row_episode)
    if span == 0 or ep[oldest] == ep[(oldest + count - 1) % H]:
        return range(span)
    chrono = np.roll(ep, -oldest)[:count]                 # rows oldest .. newest
    return np.flatnonzero(chrono[:span] == chrono[W:W + span])


def nstep_counts(row_episode, oldest, count, W, H, st, n):
    """The number of transitions m an n-step sample folds, for starts `st` (offsets from the
    oldest recorded row, each a valid one-step start): the largest m in [1, n] such that
    the one-step samples at st, st+1, .., st+m-1 are all valid — st+m-1 < count - W - 1 and
    rows st .. st+m-1+W in one episode. This is where agent/td3/td3.py:94-97 stops folding
    at `done`: an episode boundary or the newest recorded rows end the sum early."""
    st = np.asarray(st, dtype=np.int64)
    span = max(count - W - 1, 0)
    chrono = np.roll(np.asarray(row_episode), -oldest)[:count]    # rows oldest .. newest
    ok = np.zeros(span + 1, dtype=bool)                           # ok[span] = False: the newest rows end a run
    for k in range(span):
        ok[k] = np.all(chrono[k:k + W + 1] == chrono[k])
    run = np.zeros(span + 1, dtype=np.int64)                      # valid starts in a row from k on
    for k in range(span - 1, -1, -1):
        run[k] = run[k + 1] + 1 if ok[k] else 0
    if st.size and (st.min() < 0 or st.max() >= span or not ok[st].all()):
        raise ValueError("st holds a start that is not a valid one-step sample")
    return np.minimum(run[st], n).astype(np.int32)


def sequence_starts(row_episode, oldest, count, W, H, L):
    """Offsets st (from the oldest recorded row) whose sequences of L elements are full
    length, `nstep_counts(.., st, L) == L`: the one-step starts st .. st+L-1 are all valid,
    i.e. st + L - 1 < count - W - 1 and rows st .. st+L-1+W share one episode (ids only grow
    along the ring: the first and the last row decide). Returns a range when the ring holds
    one episode (every start below count - W - L), else an int64 array."""
    if L < 1:
        raise ValueError("L must be >= 1")
    span = max(count - W - L, 0)
    ep = np.asarray(row_episode)
    if span == 0 or ep[oldest] == ep[(oldest + count - 1) % H]:
        return range(span)
    chrono = np.roll(ep, -oldest)[:count]                 # rows oldest .. newest
    return np.flatnonzero(chrono[:span] == chrono[W + L - 1:W + L - 1 + span])


def valid_pairs(env_episode, oldest, count, need, H):
    """The valid (st, env) pairs of a per-env ring, int64 [total, 2] in (st ascending, env
    ascending) order: st an offset from the oldest recorded row, below span = max(count -
    need, 0), whose rows st .. st + need - 1 share one episode in column env. env_episode
    [H, B] holds ids that never decrease along the ring for one env, so the first and the
    last row decide: column b is `valid_starts(env_episode[:, b], ..)` for need = W + 1 and
    `sequence_starts(.., L)` for need = W + L. No torch, no device: this is the statement
    pmenv_replay_valid_build / _select are held to (select's k-th pair is row k)."""
    ep = np.asarray(env_episode)
    ep = ep.reshape(H, -1)
    span = max(count - need, 0)
    chrono = np.roll(ep, -oldest, axis=0)[:count]         # rows oldest .. newest
    st, env = np.nonzero(chrono[:span] == chrono[need - 1:need - 1 + span])
    return np.stack([st, env], axis=1).astype(np.int64)


def valid_build(env_episode, oldest, count, need, out=None):
    """pmenv_replay_valid_build for env_episode [H, B] int32 on the device: (bits int64
    [span, ceil(B / 64)] — the u64 words — , rowsum int64 [span + 1]). out: preallocated
    (bits, rowsum)."""
    H, B = env_episode.shape
    span, WB = max(count - need, 0), (B + 63) // 64
    if out is None:
        out = (torch.empty(span, WB, dtype=torch.int64, device=env_episode.device),
               torch.empty(span + 1, dtype=torch.int64, device=env_episode.device))
    bits, rowsum = out
    _abi.check(_abi.load().pmenv_replay_valid_build(_p(env_episode), H, B, oldest, count, need,
                                                    _p(bits) if span else None, _p(rowsum),
                                                    _stream(env_episode.device)), None, "pmenv_replay_valid_build")
    return bits, rowsum


def valid_select(bits, rowsum, H, B, oldest, u, out=None):
    """pmenv_replay_valid_select for targets u [S] f64 on the device: (h0, env) int32 [S]."""
    S, dev, span = u.numel(), rowsum.device, rowsum.numel() - 1
    if out is None:
        out = (torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.int32, device=dev))
    h0, env = out
    _abi.check(_abi.load().pmenv_replay_valid_select(_p(bits) if span else None, _p(rowsum), H, B, oldest, span,
                                                     _p(u), S, _p(h0), _p(env), _stream(dev)),
               None, "pmenv_replay_valid_select")
    return h0, env


def prio_row_events(row_episode, head, count, episode, W, H):
    """The leaves one `add` changes, decided on the host from the ring state BEFORE the add
    (row ids, head, count) — no torch, no device: (close_row or None, open_row or None).
    close_row is the ring row about to be overwritten (a full ring loses its oldest start).
    open_row is the start at offset count' - W - 2 of the ring after the add, the only start
    the new row can complete, and only when its rows st .. st + W share one episode. Those
    rows were all recorded before this add (a start's window ends one row short of the
    newest, `valid_starts`), so `episode`, the id of the row being added, decides nothing;
    it is part of the state the caller hands over. After every add the open rows are
    exactly {(oldest + st) % H : st in valid_starts(..)}."""
    close_row = head if count == H else None
    count2 = min(count + 1, H)
    oldest2 = (head + 1 - count2) % H
    st = count2 - W - 2
    open_row = None
    if st >= 0:
        first, last = (oldest2 + st) % H, (oldest2 + st + W) % H
        if row_episode[first] == row_episode[last]:
            open_row = first
    return close_row, open_row


def prio_layout(leaves):
    """The byte layout of the priority tree (include/pmenv.h): {header: 0, levels: [(byte
    offset, entries, numpy dtype), ..], bytes}; level 0 is the f32 leaves, the others f64,
    each padded with zeros to a multiple of 64 entries."""
    pad = lambda n: (n + 63) // 64 * 64  # noqa: E731
    levels, off, n = [(64, leaves, np.float32)], 64 + 4 * pad(leaves), leaves
    while True:
        n = (n + 63) // 64
        levels.append((off, n, np.float64))
        off += 8 * pad(n)
        if n <= 64:
            return dict(header=0, levels=levels, bytes=off)


def gather_path(kind, N, W, F=5, n=1, S=1, aligned=3, cus=0):
    """pmenv_replay_path: the kernel instantiation and launch geometry a sample gather takes,
    e.g. "replay_gather_f5p_kernel<8,2> R=30 D=51 grid=256x1 lds=30600". kind: "one_step"
    (`gather`), "nstep" (`gather_nstep`, n = n_step), "seq" (`gather_sequences`, n = L) or
    "rollout" (pmenv_rollout_gather); aligned: bit 0 = 16-B aligned outputs, bit 1 = 16-B
    aligned series (torch allocations are both); cus: the compute units to plan for, 0 = the
    current device's. "" for a shape the gather rejects."""
    return _abi.load().pmenv_replay_path(_abi.REPLAY_KINDS[kind], N, F, W, n, S, aligned, cus).decode()


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def prio_tree(leaves, device):
    """A zeroed tree buffer for `leaves` leaves with the maximum at 1 (pmenv_prio_init)."""
    lib = _abi.load()
    nbytes = lib.pmenv_prio_tree_bytes(leaves)
    if nbytes == 0:
        raise ValueError("leaves must be in [1, 2^31)")
    tree = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _abi.check(lib.pmenv_prio_init(_p(tree), leaves, _stream(tree.device)), None, "pmenv_prio_init")
    return tree


def prio_fill(tree, leaves, close_first, open_first, n):
    """pmenv_prio_fill: n leaves from close_first become 0, n from open_first the maximum
    (None: that range is absent)."""
    _abi.check(_abi.load().pmenv_prio_fill(_p(tree), leaves, -1 if close_first is None else close_first,
                                           -1 if open_first is None else open_first, n, _stream(tree.device)),
               None, "pmenv_prio_fill")


def prio_fill_env(tree, leaves, close_first, open_first, n, ep_first, ep_last):
    """pmenv_prio_fill_env: `prio_fill` whose open range takes only the leaves i with
    ep_first[i] == ep_last[i] (int32 [n] on the device)."""
    _abi.check(_abi.load().pmenv_prio_fill_env(_p(tree), leaves, -1 if close_first is None else close_first,
                                               -1 if open_first is None else open_first, n, _p(ep_first),
                                               _p(ep_last), _stream(tree.device)), None, "pmenv_prio_fill_env")


def prio_sample(tree, leaves, B, u, beta, out=None):
    """pmenv_prio_sample for targets u [S] f64 in [0, 1): (leaf, h0, env int32, weights f32).
    out: the four preallocated outputs (a captured graph's buffers)."""
    S, dev = u.numel(), tree.device
    if out is None:
        out = tuple(torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3)) + (
            torch.empty(S, dtype=torch.float32, device=dev),)
    leaf, h0, env, w = out
    _abi.check(_abi.load().pmenv_prio_sample(_p(tree), leaves, B, _p(u), S, float(beta), _p(leaf), _p(h0), _p(env),
                                             _p(w), _stream(dev)), None, "pmenv_prio_sample")
    return leaf, h0, env, w


def prio_update(tree, leaves, leaf, td, alpha, eps):
    """pmenv_prio_update: leaf int32 [S], td f32 [S]."""
    _abi.check(_abi.load().pmenv_prio_update(_p(tree), leaves, _p(leaf), _p(td), leaf.numel(), float(alpha),
                                             float(eps), _stream(tree.device)), None, "pmenv_prio_update")


class DeviceReplay:
    def __init__(self, num_envs, num_assets, window, capacity, series, features=5, prioritized=False, alpha=0.6,
                 beta=0.4, beta_increment=0.0, eps=1e-6, per_env=False):
        """per_env: the envs end their episodes on their own (`add(.., done=)`, the mask
        `TradingEnv.restart` returns): `env_episode` [H, B] int32 holds an id per (row, env)
        on the device and every sampling kind draws from the valid (start, env) pairs
        (`valid_pairs`). Default: the envs record in lockstep, one id per ring row.
        prioritized (agent/td3/td3.py:39 PrioritizedReplayBuffer(buffer_size, alpha, beta,
        beta_incr)): keep a priority tree over the H * B one-step starts, current after every
        `add`; `sample_prioritized` / `sample_nstep_prioritized` draw from it and
        `update_priorities` feeds the TD errors back. Sequence samples stay uniform: a
        sequence start has another validity set than a one-step start."""
        if capacity < window + 2:
            raise ValueError("capacity must hold at least window + 2 steps")
        if prioritized and (alpha < 0 or not 0.0 <= beta <= 1.0 or beta_increment < 0 or eps < 0):
            raise ValueError("alpha, beta_increment, eps must be >= 0 and beta in [0, 1]")
        if prioritized and capacity * num_envs >= 2 ** 31:
            raise ValueError("a prioritized replay holds fewer than 2^31 transitions")
        self.B, self.N, self.W, self.F, self.H = num_envs, num_assets, window, features, capacity
        self.series = series
        dev = series.device
        self.days = torch.zeros(capacity, num_envs, dtype=torch.int32, device=dev)
        self.actions = torch.zeros(capacity, num_envs, num_assets, dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(capacity, num_envs, dtype=torch.float32, device=dev)
        self.head = 0
        self.count = 0
        # episode id of every ring row (all envs record in lockstep, so one id per row)
        self.episode = 0
        self._row_ep = np.zeros(capacity, dtype=np.int64)
        self._starts = None           # device tensor of valid starts when some windows straddle episodes
        self._starts_key = None
        # the same ids on the device for the n-step gather, uploaded when a sample finds them stale
        self._row_ep_dev = torch.zeros(capacity, dtype=torch.int32, device=dev)
        self._row_ep_dirty = False
        self._seq_starts = None       # as _starts, for full-length sequence starts (the key holds L)
        self._seq_key = None
        self.prioritized = bool(prioritized)
        self.alpha, self.beta, self.beta_increment, self.eps = alpha, beta, beta_increment, eps
        self._leaves = capacity * num_envs
        self._row_open = np.zeros(capacity, dtype=bool)   # ring rows whose leaves are open (valid starts), kept by add
        self.tree = prio_tree(self._leaves, dev) if prioritized else None
        self.per_env = bool(per_env)
        if self.per_env:
            # the ids and the id the next row of each env takes live on the device alone
            self.env_episode = torch.zeros(capacity, num_envs, dtype=torch.int32, device=dev)
            self._cur = torch.zeros(num_envs, dtype=torch.int32, device=dev)
            self._adds = 0                # rows recorded so far: never repeats, unlike (head, count) of a full ring
            self._valid_at = None         # the _adds the cached maps were built at
            self._valid_maps = {}         # need -> (bits, rowsum, total)
            self._row_ep = self._row_open = None   # lockstep's host copies: not kept in this mode

    def __len__(self):
        return self.count

    def new_episode(self):
        """Steps added from now on belong to a new episode (the env was reset): no sampled
        window spans the boundary (buffer.py keeps each epoch in its own row)."""
        self.episode += 1
        if self.per_env:
            self._cur += 1

    def _add_per_env(self, day, action, reward, done):
        """`add` with an id per (row, env): plain torch and one tree launch, no sync."""
        h, H, W, B = self.head, self.H, self.W, self.B
        self.days[h].copy_(torch.as_tensor(day).reshape(B))
        self.actions[h].copy_(torch.as_tensor(action).reshape(B, self.N))
        self.rewards[h].copy_(torch.as_tensor(reward).reshape(B))
        self.env_episode[h].copy_(self._cur)
        if done is not None:
            self._cur += (torch.as_tensor(done).to(self._cur.device).reshape(B) != 0).to(torch.int32)
        full = self.count == H
        self._adds += 1                   # the cached valid maps describe the ids before this row
        self._valid_at, self._valid_maps = None, {}
        self.head = (h + 1) % H
        self.count = min(self.count + 1, H)
        if self.prioritized:
            # the overwritten row's starts close; the start at offset count' - W - 2, the only
            # one the new row completes, opens for the envs whose window lies in one episode
            oldest = (self.head - self.count) % H
            st = self.count - W - 2
            close = h * B if full else None
            if st >= 0:
                first, last = (oldest + st) % H, (oldest + st + W) % H
                prio_fill_env(self.tree, self._leaves, close, first * B, B, self.env_episode[first],
                              self.env_episode[last])
            elif close is not None:
                prio_fill(self.tree, self._leaves, close, None, B)

    def _valid(self, need):
        """The valid-pair map for `need` rows of one episode: (bits, rowsum, total), cached
        until the next add — `add` drops the maps, and they are keyed by the count of rows ever
        recorded, since (head, count) of a full ring comes round again every H adds. A rebuild
        reads the total back: 8 bytes, the only host read."""
        at = self._adds
        if self._valid_at != at:
            self._valid_at, self._valid_maps = at, {}
        hit = self._valid_maps.get(need)
        if hit is None:
            oldest = (self.head - self.count) % self.H
            bits, rowsum = valid_build(self.env_episode, oldest, self.count, need)
            hit = self._valid_maps[need] = (bits, rowsum, int(rowsum[-1].item()))
        return hit

    def _draw(self, need, batch_size, generator, u):
        """S uniform draws from the valid pairs of `need` (total > 0): (h0, env) int32."""
        bits, rowsum, _ = self._valid(need)
        dev = self.days.device
        if u is None:
            gdev = generator.device if generator is not None else dev
            u = torch.rand(batch_size, dtype=torch.float64, generator=generator, device=gdev)
        u = torch.as_tensor(u, dtype=torch.float64).to(dev).reshape(batch_size).contiguous()
        return valid_select(bits, rowsum, self.H, self.B, (self.head - self.count) % self.H, u)

    def add(self, day, action, reward, done=None):
        """buffer.py:23-37: one recorded step for every env. done [B] (per_env only; uint8 or
        bool, the mask `TradingEnv.restart` returns): env b's episode ended with this step,
        its next row opens a new one; None: no env ended."""
        if self.per_env:
            return self._add_per_env(day, action, reward, done)
        if done is not None:
            raise ValueError("done= needs a replay built with per_env=True")
        h = self.head
        if self.prioritized:              # from the state before the add
            close_row, open_row = prio_row_events(self._row_ep, h, self.count, self.episode, self.W, self.H)
        self.days[h].copy_(torch.as_tensor(day).reshape(self.B))
        self.actions[h].copy_(torch.as_tensor(action).reshape(self.B, self.N))
        self.rewards[h].copy_(torch.as_tensor(reward).reshape(self.B))
        self._row_ep_dirty |= self._row_ep[h] != self.episode
        self._row_ep[h] = self.episode
        self.head = (h + 1) % self.H
        self.count = min(self.count + 1, self.H)
        if self.prioritized:
            if close_row is not None:     # the host's copy of which rows are open: no device read to count them
                self._row_open[close_row] = False
            if open_row is not None:
                self._row_open[open_row] = True
            if close_row is not None or open_row is not None:
                prio_fill(self.tree, self._leaves, None if close_row is None else close_row * self.B,
                          None if open_row is None else open_row * self.B, self.B)

    def indices(self, batch_size, generator=None, u=None):
        """Random (start, env) pairs with W+1 consecutive recorded steps of one episode
        (buffer.py:47-51). per_env: pair floor(u * total) of `valid_pairs(.., W + 1)`, u [S]
        f64 in [0, 1) drawn with the generator (an explicit u makes the draw exact)."""
        span = self.count - self.W - 1
        if span < 1:
            raise ValueError("not enough recorded steps to sample a window")
        if self.per_env:
            if self._valid(self.W + 1)[2] == 0:
                raise ValueError("no episode holds W + 1 recorded steps")
            return self._draw(self.W + 1, batch_size, generator, u)
        if u is not None:
            raise ValueError("u= needs a replay built with per_env=True")
        # drawn where the generator lives: a CPU generator (reproducible across devices)
        # costs a host->device copy per batch; no generator or a device one stays on the GPU
        dev = self.days.device
        gdev = generator.device if generator is not None else dev
        oldest = (self.head - self.count) % self.H
        first, last = int(self._row_ep[oldest]), int(self._row_ep[(oldest + self.count - 1) % self.H])
        key = None if first == last else (oldest, self.count, first, last)
        if key is None:                    # one episode in the ring: every start (no scan, no upload)
            self._starts_key, self._starts = None, None
        elif self._starts_key != key:
            self._starts_key = key
            ok = valid_starts(self._row_ep, oldest, self.count, self.W, self.H)
            if len(ok) == 0:
                raise ValueError("no episode holds W + 1 recorded steps")
            self._starts = None if len(ok) == span else torch.as_tensor(ok, dtype=torch.int64).to(gdev)
        if self._starts is None:
            st = torch.randint(0, span, (batch_size,), generator=generator, device=gdev)
        else:
            if self._starts.device != torch.device(gdev):
                self._starts = self._starts.to(gdev)
            st = self._starts[torch.randint(0, self._starts.numel(), (batch_size,), generator=generator, device=gdev)]
        env = torch.randint(0, self.B, (batch_size,), generator=generator, device=gdev)
        h0 = (oldest + st) % self.H
        return h0.to(dev, torch.int32), env.to(dev, torch.int32)

    def gather(self, h0, env):
        """buffer.py:53-79 for the given samples: (s, a, r, s_next) shaped like the reference."""
        lib = _abi.load()
        S = h0.numel()
        dev = self.days.device
        s = torch.empty(S, self.N, self.W, self.F, device=dev)
        s2 = torch.empty_like(s)
        a = torch.empty(S, self.N, device=dev)
        r = torch.empty(S, device=dev)
        sb = self.series.bars
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _abi.check(lib.pmenv_replay_gather(_p(sb), sb.shape[0], self.N, self.F, self.W, _p(self.days),
                                           _p(self.actions), _p(self.rewards), self.H, self.B,
                                           _p(h0.contiguous()), _p(env.contiguous()), S, _p(s), _p(s2), _p(a), _p(r),
                                           st), None, "pmenv_replay_gather")
        return s, a.reshape(S, self.N, 1), r.reshape(S, 1, 1), s2

    def sample(self, batch_size, generator=None):
        return self.gather(*self.indices(batch_size, generator))

    def gather_nstep(self, h0, env, n_step, gamma):
        """The n-step transition of agent/td3/td3.py:85-106 for the given one-step samples:
        (s, a, R, s_next, steps, discount). s and a are `gather`'s; R folds the rewards of
        the m = steps[j] <= n_step transitions from h0 on, R = sum_k gamma^k r_k; s_next is
        the next state of the last folded one; discount = gamma^m is what the caller's
        bootstrap term takes. The fold stops where td3's `done` would: at an episode
        boundary and at the newest recorded rows (`nstep_counts`)."""
        lib = _abi.load()
        S = h0.numel()
        dev = self.days.device
        if self._row_ep_dirty:
            self._row_ep_dev.copy_(torch.from_numpy(self._row_ep.astype(np.int32)))
            self._row_ep_dirty = False
        fn, ids = ((lib.pmenv_replay_gather_nstep_env, self.env_episode) if self.per_env else
                   (lib.pmenv_replay_gather_nstep, self._row_ep_dev))
        s = torch.empty(S, self.N, self.W, self.F, device=dev)
        s2 = torch.empty_like(s)
        a = torch.empty(S, self.N, device=dev)
        r = torch.empty(S, device=dev)
        steps = torch.empty(S, dtype=torch.int32, device=dev)
        disc = torch.empty(S, device=dev)
        sb = self.series.bars
        oldest = (self.head - self.count) % self.H
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _abi.check(fn(_p(sb), sb.shape[0], self.N, self.F, self.W, _p(self.days), _p(self.actions), _p(self.rewards),
                      self.H, self.B, _p(h0.contiguous()), _p(env.contiguous()), S, _p(ids), oldest, self.count,
                      int(n_step), float(gamma), _p(s), _p(s2), _p(a), _p(r), _p(steps), _p(disc), st),
                   None, "pmenv_replay_gather_nstep_env" if self.per_env else "pmenv_replay_gather_nstep")
        return s, a.reshape(S, self.N, 1), r.reshape(S, 1, 1), s2, steps, disc

    def sample_nstep(self, batch_size, n_step, gamma=0.997, generator=None):
        """`sample` with n-step returns (gamma: config/dsac.py:30)."""
        return self.gather_nstep(*self.indices(batch_size, generator), n_step, gamma)

    def prioritized_indices(self, batch_size, generator=None, u=None):
        """`samples, idxs, weights = replay_buffer.sample(batch_size)` of agent/td3/td3.py:118,
        the index part: (h0, env, leaf, weights). Sample j descends the priority tree to the
        target u[j] * total; u [S] in [0, 1) defaults to the stratified draw (arange(S) +
        rand(S)) / S of Schaul et al. 2016, with `indices`' generator and device rules; an
        explicit u makes the draw exact. leaf = h0 * B + env is what `update_priorities` takes
        back; weights [S] f32 = (N P(j))^-beta / max_k w_k with the current beta, which then
        advances by beta_increment, capped at 1 (td3.py:39 beta_incr)."""
        if not self.prioritized:
            raise ValueError("the replay was built with prioritized=False")
        if self.count - self.W - 1 < 1:
            raise ValueError("not enough recorded steps to sample a window")
        if self.per_env:
            empty = self._valid(self.W + 1)[2] == 0
        else:
            empty = not self._row_open.any()
        if empty:
            raise ValueError("no episode holds W + 1 recorded steps")
        dev = self.days.device
        if u is None:
            gdev = generator.device if generator is not None else dev
            u = (torch.arange(batch_size, dtype=torch.float64, device=gdev) +
                 torch.rand(batch_size, dtype=torch.float64, generator=generator, device=gdev)) / batch_size
        u = torch.as_tensor(u, dtype=torch.float64).to(dev).reshape(batch_size).contiguous()
        beta = self.beta
        self.beta = min(1.0, beta + self.beta_increment)
        leaf, h0, env, w = prio_sample(self.tree, self._leaves, self.B, u, beta)
        return h0, env, leaf, w

    def sample_prioritized(self, batch_size, generator=None, u=None):
        """`sample` drawn by priority: (s, a, r, s_next, leaf, weights)."""
        h0, env, leaf, w = self.prioritized_indices(batch_size, generator, u)
        return self.gather(h0, env) + (leaf, w)

    def sample_nstep_prioritized(self, batch_size, n_step, gamma=0.997, generator=None, u=None):
        """`sample_nstep` drawn by priority: (s, a, R, s_next, steps, discount, leaf, weights)."""
        h0, env, leaf, w = self.prioritized_indices(batch_size, generator, u)
        return self.gather_nstep(h0, env, n_step, gamma) + (leaf, w)

    def update_priorities(self, leaf, td_error):
        """replay_buffer.update_priorities(idxs, td_error) of agent/td3/td3.py:144: leaf j takes
        (|td_error[j]| + eps)^alpha. A leaf whose row was overwritten or closed since it was
        sampled stays closed; of repeated leaves the largest value wins."""
        if not self.prioritized:
            raise ValueError("the replay was built with prioritized=False")
        dev = self.days.device
        leaf = torch.as_tensor(leaf).to(dev, torch.int32).reshape(-1).contiguous()
        td = torch.as_tensor(td_error).detach().to(dev, torch.float32).reshape(-1).contiguous()
        if td.numel() != leaf.numel():
            raise ValueError("leaf and td_error must hold one value per sample")
        prio_update(self.tree, self._leaves, leaf, td, self.alpha, self.eps)


    def sequence_indices(self, batch_size, L, generator=None, u=None):
        """Random (start, env) pairs whose sequences of L consecutive one-step samples are
        full length: W + L recorded rows of one episode (`sequence_starts`). The generator
        and device rules are those of `indices`, and so are per_env's draw and u, over
        `valid_pairs(.., W + L)`."""
        if L < 1:
            raise ValueError("L must be >= 1")
        span = self.count - self.W - L
        if span < 1:
            raise ValueError("no episode holds W + L recorded steps")
        if self.per_env:
            if self._valid(self.W + int(L))[2] == 0:
                raise ValueError("no episode holds W + L recorded steps")
            return self._draw(self.W + int(L), batch_size, generator, u)
        if u is not None:
            raise ValueError("u= needs a replay built with per_env=True")
        dev = self.days.device
        gdev = generator.device if generator is not None else dev
        oldest = (self.head - self.count) % self.H
        first, last = int(self._row_ep[oldest]), int(self._row_ep[(oldest + self.count - 1) % self.H])
        if first == last:                  # one episode in the ring: every start (no scan, no upload)
            self._seq_key, self._seq_starts = None, None
            st = torch.randint(0, span, (batch_size,), generator=generator, device=gdev)
        else:
            key = (oldest, self.count, first, last, L)
            if self._seq_key != key:
                ok = sequence_starts(self._row_ep, oldest, self.count, self.W, self.H, L)
                self._seq_key, self._seq_starts = key, torch.as_tensor(np.asarray(ok), dtype=torch.int64).to(gdev)
            if self._seq_starts.numel() == 0:
                raise ValueError("no episode holds W + L recorded steps")
            if self._seq_starts.device != torch.device(gdev):
                self._seq_starts = self._seq_starts.to(gdev)
            st = self._seq_starts[torch.randint(0, self._seq_starts.numel(), (batch_size,), generator=generator,
                                                device=gdev)]
        env = torch.randint(0, self.B, (batch_size,), generator=generator, device=gdev)
        h0 = (oldest + st) % self.H
        return h0.to(dev, torch.int32), env.to(dev, torch.int32)

    def gather_sequences(self, h0, env, L, time_major=True):
        """Sequences of L consecutive one-step samples from the given valid one-step starts:
        (x, a, r, length). Element t of sequence j is `gather`'s (s, a, r) at start h0[j] + t.
        time_major: x [L, S, N, W, F], a [L, S, N], r [L, S] (world_model.py:41-64 walks
        [batch_len, batch_dim, ..]); else x [S, L, N, W, F], a [S, L, N], r [S, L]. length [S]
        int32 is the number of valid elements — an episode boundary or the newest recorded
        rows cut a sequence short (`nstep_counts` with n = L) — and the elements behind it
        are zeros: length is the caller's mask."""
        lib = _abi.load()
        S, L = h0.numel(), int(L)
        dev = self.days.device
        if self._row_ep_dirty:
            self._row_ep_dev.copy_(torch.from_numpy(self._row_ep.astype(np.int32)))
            self._row_ep_dirty = False
        fn, ids = ((lib.pmenv_replay_gather_seq_env, self.env_episode) if self.per_env else
                   (lib.pmenv_replay_gather_seq, self._row_ep_dev))
        lead = (L, S) if time_major else (S, L)
        x = torch.empty(*lead, self.N, self.W, self.F, device=dev)
        a = torch.empty(*lead, self.N, device=dev)
        r = torch.empty(*lead, device=dev)
        length = torch.empty(S, dtype=torch.int32, device=dev)
        sb = self.series.bars
        oldest = (self.head - self.count) % self.H
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _abi.check(fn(_p(sb), sb.shape[0], self.N, self.F, self.W, _p(self.days), _p(self.actions), _p(self.rewards),
                      self.H, self.B, _p(h0.contiguous()), _p(env.contiguous()), S, _p(ids), oldest, self.count, L,
                      1 if time_major else 0, _p(x), _p(a), _p(r), _p(length), st), None,
                   "pmenv_replay_gather_seq_env" if self.per_env else "pmenv_replay_gather_seq")
        return x, a, r, length

    def sample_sequences(self, batch_size, L, generator=None, time_major=True):
        """A batch of full-length sequences for DreamerV3's world model:
        agent/dreamer/dreamer.py:78 reads `x, a, r = data["x"], data["a"], data["r"]` — x the
        observation windows, a the actions taken on them, r their rewards, [batch_len,
        batch_dim, ..] with config/dreamer.py:4-5's BATCH_DIM = batch_size and BATCH_LEN = L.
        Returns (x, a, r, length) as `gather_sequences`; every length is L."""
        return self.gather_sequences(*self.sequence_indices(batch_size, L, generator), L, time_major)


def trajectory_metrics(returns, values, weights, risk_free_rate=RISK_FREE_RATE, periods=252):
    """Per-env {sharpe, sortino, max_drawdown, average_turnover, final_value} over a
    trajectory: returns [T, B] simple returns, values [T+1, B], weights [T+1, B, N]."""
    lib = _abi.load()
    r = returns.to(torch.float64).contiguous()
    T, B = r.shape
    v = values.to(device=r.device, dtype=torch.float64).contiguous()
    w = weights.to(device=r.device, dtype=torch.float32).contiguous()
    if tuple(v.shape) != (T + 1, B) or w.shape[:2] != (T + 1, B):
        raise ValueError("values must be [T+1, B] and weights [T+1, B, N]")
    out = torch.empty(B, 5, dtype=torch.float64, device=r.device)
    st = ctypes.c_void_p(torch.cuda.current_stream(r.device).cuda_stream)
    _abi.check(lib.pmenv_metrics(_p(r), _p(v), _p(w), T, B, w.shape[2], float(risk_free_rate), float(periods),
                                 _p(out), st), None, "pmenv_metrics")
    keys = ("sharpe", "sortino", "max_drawdown", "average_turnover", "final_value")
    return {k: out[:, i] for i, k in enumerate(keys)}


def episode_metrics(returns, values, weights, dones, init_value, max_episodes=None, risk_free_rate=RISK_FREE_RATE,
                    periods=252):
    """`trajectory_metrics` per episode, for envs that end their episodes on their own
    (pmenv.episodes): returns [T, B], values [T+1, B], weights [T+1, B, N] as above — a row
    that ended an episode holds the terminal value and weights, taken before the restart — and
    dones [T, B] (bool / uint8, any nonzero byte: that step ended env b's episode). A restarted
    env begins from `init_value` and the weights e0. Env b's record is cut into count[b] >= 1
    episodes, the last one open unless the last row is a done (include/pmenv.h has the contract).
    Returns {sharpe, sortino, max_drawdown, average_turnover, final_value: [B, K] f64, first,
    last: [B, K] int32 (steps 1 .. T), count: [B] int32}; episodes k < min(count[b], K) in
    chronological order, NaN / 0 in the slots past them; count is exact even above K.
    max_episodes=None takes K = 1 + the most dones of any env, one host read; a caller who knows a bound
    passes it and the call reads nothing back."""
    lib = _abi.load()
    r = returns.to(torch.float64).contiguous()
    T, B = r.shape
    v = values.to(device=r.device, dtype=torch.float64).contiguous()
    w = weights.to(device=r.device, dtype=torch.float32).contiguous()
    if tuple(v.shape) != (T + 1, B) or w.shape[:2] != (T + 1, B):
        raise ValueError("values must be [T+1, B] and weights [T+1, B, N]")
    if tuple(dones.shape) != (T, B):
        raise ValueError("dones must be [T, B]")
    d = dones.to(device=r.device)
    if d.dtype != torch.uint8:                  # uint8 goes as it is: any nonzero byte is an episode end
        d = d.ne(0).to(torch.uint8)
    d = d.contiguous()
    if max_episodes is None:
        max_episodes = int(d.ne(0).sum(0).max()) + 1
    K = int(max_episodes)
    if K < 1:
        raise ValueError("max_episodes must be at least 1")
    out = torch.empty(B, K, 5, dtype=torch.float64, device=r.device)
    span = torch.empty(B, K, 2, dtype=torch.int32, device=r.device)
    count = torch.empty(B, dtype=torch.int32, device=r.device)
    st = ctypes.c_void_p(torch.cuda.current_stream(r.device).cuda_stream)
    _abi.check(lib.pmenv_metrics_episodes(_p(r), _p(v), _p(w), _p(d), T, B, w.shape[2], float(init_value),
                                          float(risk_free_rate), float(periods), K, _p(out), _p(span), _p(count),
                                          st), None, "pmenv_metrics_episodes")
    keys = ("sharpe", "sortino", "max_drawdown", "average_turnover", "final_value")
    res = {k: out[:, :, i] for i, k in enumerate(keys)}
    res.update(first=span[:, :, 0], last=span[:, :, 1], count=count)
    return res
