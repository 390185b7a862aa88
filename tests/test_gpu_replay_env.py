"""The device replay with an episode id per (row, env) (`DeviceReplay(per_env=True)`) on an
MI355X: the valid-pair map and the exact draw (pmenv_replay_valid_build / _select) against
`valid_pairs`, the n-step and sequence gathers with per-env ids against the one-step
restatement (oracle.replay_gather) composed as test_gpu_replay_nstep.py composes it, the
priority tree per env against tests/prio_ref.py, and OffPolicy(episodes=True) end to end.
Needs a GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import prio_ref
from replay_env_inputs import bits_of, done_rows, record, ring_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GAMMA = 0.9
GUARD = 0x5A5A5A5A5A5A5A5A
S_MAX = 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


SHAPES = [(4, 4, 5), (3, 3, 3), (30, 50, 5)]           # N, W, F
ENVS = [1, 64, 70, 129]
# the kernel each shape takes, asserted through gather_path before any value is compared
NSTEP_FORMS = {(4, 4, 5): "replay_nstep_f5p_kernel<", (3, 3, 3): "replay_nstep_lds_kernel",
               (30, 50, 5): "replay_nstep_f5p_kernel<", (257, 3, 5): "replay_nstep_kernel "}
SEQ_FORMS = {(4, 4, 5): "replay_seq_f5p_kernel<", (3, 3, 3): "replay_seq_kernel", (30, 50, 5): "replay_seq_f5p_kernel<",
             (257, 3, 5): "replay_seq_kernel "}
RINGS = [(s, b, w) for s in SHAPES for b in ENVS for w in (True, False)]
# N > 256 with no 16-B granular asset group: the one-thread-per-float n-step kernel, the one form
# the three shapes above do not reach (it takes the ids as runtime strides too)
GATHER_RINGS = RINGS + [((257, 3, 5), 70, True), ((257, 3, 5), 70, False)]
RING_IDS = [f"N{s[0]}-W{s[1]}-F{s[2]}-B{b}-{'wrapped' if w else 'short'}" for s, b, w in GATHER_RINGS]


def fill(rb, done, day0, seed):
    """Record done's rows: env b's day at recorded step t is day0 + t + b % 3."""
    rows, B = done.shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    off = torch.arange(B, dtype=torch.int32, device=DEV) % 3
    done_dev = torch.as_tensor(done.astype(np.uint8), device=DEV)
    for t in range(rows):
        rb.add(day0 + t + off, torch.rand(B, rb.N, device=DEV, generator=g), torch.randn(B, device=DEV, generator=g),
               done=done_dev[t])


@functools.lru_cache(maxsize=None)
def ring(N, W, F, B, wrapped, H=None, rows=None):
    """A per-env replay over heterogeneous columns (replay_env_inputs), wrapped (count == H,
    the oldest row mid-array) or short (count < H), whose days run off both ends of the
    series; the host's copy of the ids; the valid pairs for need = W + 1; up to 64 sampled
    pairs (hand-picked ones first); the one-step restatement at them. Computed once."""
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay, nstep_counts, valid_pairs
    from oracle import replay_gather
    if H is None:
        H, rows = ring_rows(W, wrapped)
    done = done_rows(rows, B, W, seed=100 * W + B)
    ep, head, count = record(done, H)
    wide = H < 4 * W + 9                                                      # the B = 4,160 ring: map and draws only
    T = 8 if wide else count - 8
    rng = np.random.default_rng(N * 100 + W)
    bars = (100 * np.exp(0.01 * rng.standard_normal((T, N, F - 1)).cumsum(0))).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV), features=F, per_env=True)
    fill(rb, done, -3 - (rows - count), seed=N + W + B)
    oldest = (head - count) % H
    # the fixture's preconditions, on the host
    assert (rb.head, rb.count) == (head, count)
    assert (count == H and oldest > 0) if wrapped else (count < H and oldest == 0)
    span = count - W - 1
    pairs = valid_pairs(ep, oldest, count, W + 1, H)
    assert len(pairs) > 0 and (pairs[:, 1] == 0).sum() == span                # total > 0; env 0 never ends
    if B > 1:
        assert not (pairs[:, 1] == 1).any()                                   # env 1 ends every row
    if B > 2:
        assert 1 <= (pairs[:, 1] == 2).sum() <= span // (W + 1) + 1           # env 2: one start per episode
    env0 = np.flatnonzero(pairs[:, 1] == 0)
    picked = [env0[0], env0[1], env0[-1], env0[-2], env0[-3]] + list(np.flatnonzero(pairs[:, 1] == 2)[:4])
    rest = np.random.default_rng(B).permutation(len(pairs))[:S_MAX - len(picked)]
    sel = pairs[np.concatenate([np.array(picked, dtype=np.int64), rest])]
    st, env = sel[:, 0], sel[:, 1].astype(np.int32)
    h0 = ((oldest + st) % H).astype(np.int32)
    S = len(st)

    def counts(n):                                                            # per column, today's definition
        m = np.empty(S, np.int32)
        for b in np.unique(env):
            m[env == b] = nstep_counts(ep[:, b], oldest, count, W, H, st[env == b], n)
        return m
    days, actions, rewards = rb.days.cpu().numpy(), rb.actions.cpu().numpy(), rb.rewards.cpu().numpy()
    dl = days[(h0 + W - 1) % H, env]
    assert wide or (dl - (W - 1) < 0).any() and (dl + 1 >= T).any()          # windows off both ends of the series
    one = None if wide else replay_gather(bars, days, actions, rewards, h0, env, W)
    return dict(rb=rb, bars=bars, ep=ep, H=H, T=T, oldest=oldest, count=count, span=span, pairs=pairs, st=st, env=env,
                h0=h0, S=S, counts=counts, run=counts(10 ** 6), days=days, actions=actions, rewards=rewards, one=one,
                h0_dev=torch.as_tensor(h0, device=DEV), env_dev=torch.as_tensor(env, device=DEV))


def wide_ring(wrapped):
    """B = 4,160: 65 words per row, so the select's scan takes a second round."""
    return ring(2, 2, 5, 4160, wrapped, 8, 8 + 3 if wrapped else 6)


MAP_RINGS = [(s[1], b, w) for s in SHAPES for b in ENVS for w in (True, False)] + [(2, 4160, True), (2, 4160, False)]
MAP_IDS = [f"W{w}-B{b}-{'wrapped' if wr else 'short'}" for w, b, wr in MAP_RINGS]


def map_ring(W, B, wrapped):
    if B == 4160:
        return wide_ring(wrapped)
    N, _, F = next(s for s in SHAPES if s[1] == W)
    return ring(N, W, F, B, wrapped)


def guarded(n):
    """An int64 buffer of n words between two runs of 8 guard words: (whole, view)."""
    whole = torch.full((n + 16,), GUARD, dtype=torch.int64, device=DEV)
    return whole, whole[8:8 + n]


def guards_intact(whole, n):
    w = whole.cpu().numpy()
    return (w[:8] == GUARD).all() and (w[8 + n:] == GUARD).all()


@pytest.mark.parametrize("W,B,wrapped", MAP_RINGS, ids=MAP_IDS)
def test_gpu_valid_map_matches_numpy(W, B, wrapped):
    from pmenv import _abi
    from pmenv.replay import valid_pairs
    c = map_ring(W, B, wrapped)
    rb, H, count, oldest = c["rb"], c["H"], c["count"], c["oldest"]
    assert np.array_equal(rb.env_episode.cpu().numpy(), c["ep"])             # add(done=) recorded the ids
    lib, WB = _abi.load(), (B + 63) // 64
    for need in (W + 1, W + 2, W + W, count + 1):                            # count + 1: a need above count
        span = max(count - need, 0)
        pairs = valid_pairs(c["ep"], oldest, count, need, H)
        ebits, erow = bits_of(pairs, span, B)
        if need <= W + 2:
            assert len(pairs) > 0
        if need > count:
            assert span == 0 and len(pairs) == 0
        wb, bits = guarded(max(span, 1) * WB)
        wr, rowsum = guarded(span + 1)
        rc = lib.pmenv_replay_valid_build(P(rb.env_episode), H, B, oldest, count, need, P(bits), P(rowsum), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert guards_intact(wb, max(span, 1) * WB) and guards_intact(wr, span + 1)
        got_row = rowsum.cpu().numpy()
        assert np.array_equal(got_row, erow) and got_row[-1] == len(pairs)
        got_bits = bits.cpu().numpy().view(np.uint64)
        if span == 0:
            assert (got_bits == np.uint64(GUARD)).all()                      # nothing else written
        else:
            assert np.array_equal(got_bits.reshape(span, WB), ebits)         # the padding bits are zero in ebits


@pytest.mark.parametrize("W,B,wrapped", MAP_RINGS, ids=MAP_IDS)
def test_gpu_valid_select_is_exact(W, B, wrapped):
    from pmenv.replay import valid_build, valid_pairs, valid_select
    c = map_ring(W, B, wrapped)
    rb, H, count, oldest = c["rb"], c["H"], c["count"], c["oldest"]
    for need in (W + 1, W + W):
        pairs = valid_pairs(c["ep"], oldest, count, need, H)
        total = len(pairs)
        bits, rowsum = valid_build(rb.env_episode, oldest, count, need)
        if total == 0:
            continue
        ks = np.arange(0, total, 7 if B == 4160 else 1, dtype=np.int64)      # every k; a stride at B = 4,160
        ks = np.union1d(ks, [total - 1])
        u = np.concatenate([(ks + 0.5) / total, [0.0, np.nextafter(1.0, 0.0), np.nan, -1.0, 2.0]])
        want = np.concatenate([pairs[ks], pairs[[0, -1, 0, 0, -1]]])
        h0, env = valid_select(bits, rowsum, H, B, oldest, torch.as_tensor(u, device=DEV))
        assert h0.dtype == env.dtype == torch.int32
        assert np.array_equal(env.cpu().numpy(), want[:, 1])
        assert np.array_equal(h0.cpu().numpy(), (oldest + want[:, 0]) % H)
    assert B != 4160 or (B + 63) // 64 > 64                                   # the scan's second round is reached
    if B == 4160:
        assert (valid_pairs(c["ep"], oldest, count, W + 1, H)[:, 1] >= 4096).any()


def test_gpu_valid_select_of_an_empty_map_and_the_python_errors():
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay, valid_build, valid_select
    N, W, B, H = 4, 4, 5, 25
    bars = np.random.default_rng(0).standard_normal((40, N, 4)).astype(np.float32)
    done = np.ones((12, B), dtype=bool)                                       # every env ends every row
    for prioritized in (False, True):
        rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV), per_env=True, prioritized=prioritized)
        with pytest.raises(ValueError, match="not enough recorded steps"):
            rb.indices(4)
        fill(rb, done, 5, seed=1)
        bits, rowsum = valid_build(rb.env_episode, 0, rb.count, W + 1)
        assert int(rowsum[-1]) == 0 and not bits.any()
        whole, out = guarded(8)
        h0, env = out.view(torch.int32)[:8], out.view(torch.int32)[8:]
        valid_select(bits, rowsum, H, B, 0, torch.rand(8, dtype=torch.float64, device=DEV), out=(h0, env))
        assert (h0 == -1).all() and (env == -1).all() and guards_intact(whole, 8)
        # a need above count: span 0, total 0
        bits0, rowsum0 = valid_build(rb.env_episode, 0, rb.count, rb.count + 3)
        assert rowsum0.tolist() == [0]
        h0, env = valid_select(bits0, rowsum0, H, B, 0, torch.rand(3, dtype=torch.float64, device=DEV))
        assert (h0 == -1).all() and (env == -1).all()
        with pytest.raises(ValueError, match=r"no episode holds W \+ 1 recorded steps"):
            rb.indices(4)
        with pytest.raises(ValueError, match=r"no episode holds W \+ 1 recorded steps"):
            rb.sample_nstep(4, 2)
        with pytest.raises(ValueError, match=r"no episode holds W \+ L recorded steps"):
            rb.sequence_indices(4, 2)
        with pytest.raises(ValueError, match=r"no episode holds W \+ L recorded steps"):
            rb.sequence_indices(4, 12)                                        # W + L above count
        if prioritized:
            with pytest.raises(ValueError, match=r"no episode holds W \+ 1 recorded steps"):
                rb.prioritized_indices(4)
            assert not prio_ref.read_tree(rb.tree, H * B)[1][0].any()        # no leaf ever opened


@pytest.mark.parametrize("shape,B,wrapped", [r for r in RINGS if r[0] == SHAPES[0]],
                         ids=[i for r, i in zip(GATHER_RINGS, RING_IDS) if r[0] == SHAPES[0]])
def test_gpu_indices_draw_valid_pairs(shape, B, wrapped):
    from pmenv.replay import valid_pairs, valid_select
    N, W, F = shape
    c = ring(N, W, F, B, wrapped)
    rb, H, oldest = c["rb"], c["H"], c["oldest"]
    L = 3
    for need, draw in ((W + 1, lambda **kw: rb.indices(200, **kw)), (W + L, lambda **kw: rb.sequence_indices(200, L, **kw))):
        valid = set(map(tuple, valid_pairs(c["ep"], oldest, c["count"], need, H).tolist()))
        assert valid
        for gen in (None, torch.Generator().manual_seed(3), torch.Generator(device=DEV).manual_seed(3)):
            h0, env = draw(generator=gen)
            assert h0.dtype == env.dtype == torch.int32 and h0.device.type == "cuda"
            got = set(zip(((h0.cpu().numpy().astype(np.int64) - oldest) % H).tolist(), env.cpu().numpy().tolist()))
            assert got <= valid and (len(valid) < 4 or len(got) > 1)
        a = draw(generator=torch.Generator().manual_seed(5))
        b = draw(generator=torch.Generator().manual_seed(5))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])            # the generator decides the draw
        u = torch.rand(200, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
        bits, rowsum, total = rb._valid(need)
        assert total == len(valid)
        want = valid_select(bits, rowsum, H, B, oldest, u.to(DEV))
        got = draw(u=u)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    h0, env = rb.sequence_indices(200, L)                                     # every sequence_indices draw has full length
    assert (rb.gather_sequences(h0, env, L)[3] == L).all()


def test_gpu_lockstep_indices_keep_their_draw():
    """Lockstep mode draws what the code before per-env mode drew: the host's valid starts
    indexed by torch.randint, then the env by torch.randint, under the same generator."""
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay, sequence_starts, valid_starts
    N, W, B, H = 4, 4, 6, 30
    bars = np.random.default_rng(0).standard_normal((60, N, 4)).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV))
    assert not rb.per_env and not hasattr(rb, "env_episode")
    for length in (11, 9, 16):
        rb.new_episode()
        for k in range(length):
            rb.add(torch.full((B,), 4 + k, dtype=torch.int32, device=DEV), torch.rand(B, N, device=DEV),
                   torch.randn(B, device=DEV))
    with pytest.raises(ValueError, match="per_env"):
        rb.add(torch.zeros(B, dtype=torch.int32, device=DEV), torch.rand(B, N, device=DEV), torch.randn(B, device=DEV),
               done=torch.zeros(B, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="per_env"):
        rb.indices(4, u=torch.rand(4, dtype=torch.float64))
    oldest = (rb.head - rb.count) % H
    for gdev in ("cpu", DEV):
        for L in (None, 3):
            ok = valid_starts(rb._row_ep, oldest, rb.count, W, H) if L is None else \
                sequence_starts(rb._row_ep, oldest, rb.count, W, H, L)
            ok = torch.as_tensor(np.asarray(ok), dtype=torch.int64).to(gdev)
            assert 0 < ok.numel() < rb.count - W - (1 if L is None else L)
            g = torch.Generator(device=gdev).manual_seed(11)
            st = ok[torch.randint(0, ok.numel(), (50,), generator=g, device=gdev)]
            env = torch.randint(0, B, (50,), generator=g, device=gdev)
            g2 = torch.Generator(device=gdev).manual_seed(11)
            h0, e = rb.indices(50, generator=g2) if L is None else rb.sequence_indices(50, L, generator=g2)
            assert torch.equal(h0.cpu(), ((oldest + st) % H).to(torch.int32).cpu()) and torch.equal(e.cpu(), env.to(torch.int32).cpu())
    # one episode in the ring, the commonest lockstep draw: every start, randint over the span itself
    one = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV))
    for k in range(H + 7):                                                    # wrapped, never a new_episode()
        one.add(torch.full((B,), k, dtype=torch.int32, device=DEV), torch.rand(B, N, device=DEV), torch.randn(B, device=DEV))
    oldest = (one.head - one.count) % H
    assert one.count == H and oldest > 0 and len(set(one._row_ep.tolist())) == 1
    for gdev in ("cpu", DEV):
        for L in (None, 3):
            span = one.count - W - (1 if L is None else L)
            ok = valid_starts(one._row_ep, oldest, one.count, W, H) if L is None else \
                sequence_starts(one._row_ep, oldest, one.count, W, H, L)
            assert isinstance(ok, range) and len(ok) == span                 # the shortcut: no list of starts
            g = torch.Generator(device=gdev).manual_seed(12)
            st = torch.randint(0, span, (50,), generator=g, device=gdev)
            env = torch.randint(0, B, (50,), generator=g, device=gdev)
            g2 = torch.Generator(device=gdev).manual_seed(12)
            h0, e = one.indices(50, generator=g2) if L is None else one.sequence_indices(50, L, generator=g2)
            assert one._starts is None and one._seq_starts is None
            assert torch.equal(h0.cpu(), ((oldest + st) % H).to(torch.int32).cpu()) and torch.equal(e.cpu(), env.to(torch.int32).cpu())


def test_gpu_valid_map_is_rebuilt_after_the_ring_comes_round():
    """(head, count) of a full ring repeats every H adds: a draw after exactly H adds with other
    `done` columns must come from the new ids, not from the map built H adds ago."""
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay, valid_pairs
    N, W, B = 4, 4, 70
    H = 4 * W + 9
    bars = np.random.default_rng(0).standard_normal((3 * H, N, 4)).astype(np.float32)
    for prioritized in (False, True):
        rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV), per_env=True, prioritized=prioritized)
        first = done_rows(H + 5, B, W, seed=1)
        second = done_rows(H, B, W, seed=2)[:, ::-1].copy()                  # other columns end, at other rows
        fill(rb, first, 0, seed=1)
        at = (rb.head, rb.count)
        ep0, head, count = record(first, H)
        oldest = (head - count) % H
        u = torch.as_tensor((np.arange(300) + 0.5) / 300, dtype=torch.float64)
        draws = []
        for L, need in ((None, W + 1), (3, W + 3)):
            pairs0 = valid_pairs(ep0, oldest, count, need, H)
            h0, env = rb.indices(300, u=u) if L is None else rb.sequence_indices(300, L, u=u)
            k = np.floor(u.numpy() * len(pairs0)).astype(np.int64)
            assert np.array_equal(env.cpu().numpy(), pairs0[k, 1])
            assert np.array_equal(h0.cpu().numpy(), (oldest + pairs0[k, 0]) % H)
            draws.append((h0.cpu().numpy(), env.cpu().numpy()))
        fill(rb, second, H + 5, seed=2)                                       # exactly H adds
        assert (rb.head, rb.count) == at
        ep1, head1, count1 = record(np.concatenate([first, second]), H)
        assert (head1, count1) == (head, count) and np.array_equal(rb.env_episode.cpu().numpy(), ep1)
        for (L, need), old in zip(((None, W + 1), (3, W + 3)), draws):
            pairs0, pairs1 = valid_pairs(ep0, oldest, count, need, H), valid_pairs(ep1, oldest, count, need, H)
            assert len(pairs1) > 0 and not np.array_equal(pairs0, pairs1)    # the valid set did change
            h0, env = rb.indices(300, u=u) if L is None else rb.sequence_indices(300, L, u=u)
            k = np.floor(u.numpy() * len(pairs1)).astype(np.int64)
            assert np.array_equal(env.cpu().numpy(), pairs1[k, 1])
            assert np.array_equal(h0.cpu().numpy(), (oldest + pairs1[k, 0]) % H)
            assert not (np.array_equal(h0.cpu().numpy(), old[0]) and np.array_equal(env.cpu().numpy(), old[1]))
        assert rb._valid(W + 1)[2] == len(valid_pairs(ep1, oldest, count, W + 1, H))
        if prioritized:
            h0, env, leaf, _ = rb.prioritized_indices(64, generator=torch.Generator().manual_seed(3))
            valid = set(map(tuple, valid_pairs(ep1, oldest, count, W + 1, H).tolist()))
            got = set(zip(((h0.cpu().numpy().astype(np.int64) - oldest) % H).tolist(), env.cpu().numpy().tolist()))
            assert got <= valid


def n_values(W):
    return [1, 2, W, W + 1, 2 * W + 3]


NSTEP_CASES = [(r, k) for r in GATHER_RINGS for k in range(5)]


@pytest.mark.parametrize("rg,k", NSTEP_CASES, ids=[f"{i}-n{n_values(r[0][1])[k]}" for (r, k), i in
                                                   zip(NSTEP_CASES, [x for x in RING_IDS for _ in range(5)])])
def test_gpu_nstep_per_env_matches_composed_restatement(rg, k):
    """The boundary-stopped folds need a column that ends: they are asserted where the ring
    has one (B >= 3; at B = 1 the ring is env 0 alone, which never ends)."""
    from pmenv.replay import gather_path
    from oracle import replay_gather
    (N, W, F), B, wrapped = rg
    n = n_values(W)[k]
    c = ring(N, W, F, B, wrapped)
    rb, H, h0, env, st, run, S, span = c["rb"], c["H"], c["h0"], c["env"], c["st"], c["run"], c["S"], c["span"]
    m = c["counts"](n)
    assert (m == n).any()                                                     # a full fold
    if n > 1:
        assert ((m < n) & (st + m == span)).any()                             # stopped by the newest rows
        if B >= 3:
            assert ((m < n) & (m == run) & (st + m < span)).any()             # stopped by an episode boundary
    es, ea, er1, _ = c["one"]
    _, _, _, es2 = replay_gather(c["bars"], c["days"], c["actions"], c["rewards"], (h0 + m - 1) % H, env, W)
    g64 = np.float64(np.float32(GAMMA))
    eR, ed = np.empty(S, np.float64), np.empty(S, np.float64)
    for j in range(S):
        r = c["rewards"][(h0[j] + W - 1 + np.arange(m[j])) % H, env[j]].astype(np.float64)
        acc = r[-1]
        for x in r[-2::-1]:                                                   # td3.py:94-96
            acc = x + g64 * acc
        eR[j] = acc
        ed[j] = np.prod(np.full(m[j], g64))
    assert gather_path("nstep", N, W, F, n=n, S=S).startswith(NSTEP_FORMS[N, W, F])
    s, a, R, s2, steps, disc = rb.gather_nstep(c["h0_dev"], c["env_dev"], n, GAMMA)
    assert s.shape == (S, N, W, F) and s2.shape == s.shape and a.shape == (S, N, 1) and R.shape == (S, 1, 1)
    assert np.array_equal(steps.cpu().numpy(), m)
    assert np.array_equal(s.cpu().numpy(), es, equal_nan=True)
    assert np.array_equal(s2.cpu().numpy(), es2, equal_nan=True)
    assert np.array_equal(a.cpu().numpy()[..., 0], ea)
    R, disc = R.cpu().numpy()[:, 0, 0].astype(np.float64), disc.cpu().numpy().astype(np.float64)
    assert (np.abs(R - eR) <= 1e-6 * np.abs(eR) + 1e-9).all()
    assert (np.abs(disc - ed) <= 1e-6 * np.abs(ed) + 1e-9).all()
    if n == 1:
        assert np.array_equal(R.astype(np.float32), er1)


def ibits(x):
    return np.ascontiguousarray(x).view(np.int32)


SEQ_CASES = [(r, tm) for r in GATHER_RINGS for tm in (True, False)]


@pytest.mark.parametrize("rg,time_major", SEQ_CASES, ids=[f"{i}-{'tm' if tm else 'bm'}" for (r, tm), i in
                                                          zip(SEQ_CASES, [x for x in RING_IDS for _ in range(2)])])
def test_gpu_sequences_per_env_match_one_step_restatement(rg, time_major):
    from pmenv.replay import gather_path
    from oracle import replay_gather
    (N, W, F), B, wrapped = rg
    c = ring(N, W, F, B, wrapped)
    rb, H, h0, env, st, run, S, span = c["rb"], c["H"], c["h0"], c["env"], c["st"], c["run"], c["S"], c["span"]
    for L in (1, 3, W + 2):
        m = c["counts"](L)
        assert np.array_equal(m, np.minimum(L, run)) and (m == L).any()       # length == min(L, run)
        if L > 1:
            assert ((m < L) & (st + m == span)).any()                         # cut by the newest rows
            if B >= 3:
                assert ((m < L) & (st + m < span)).any()                      # cut by an episode boundary
        live = np.arange(L)[None, :] < m[:, None]
        jj, tt = np.nonzero(live)
        s1, a1, r1, _ = replay_gather(c["bars"], c["days"], c["actions"], c["rewards"], (h0[jj] + tt) % H, env[jj], W)
        assert gather_path("seq", N, W, F, n=L, S=S).startswith(SEQ_FORMS[N, W, F])
        x, a, r, length = rb.gather_sequences(c["h0_dev"], c["env_dev"], L, time_major=time_major)
        lead = (L, S) if time_major else (S, L)
        assert x.shape == lead + (N, W, F) and a.shape == lead + (N,) and r.shape == lead
        assert np.array_equal(length.cpu().numpy(), m)
        x, a, r = x.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy()
        if time_major:
            x, a, r = x.swapaxes(0, 1), a.swapaxes(0, 1), r.swapaxes(0, 1)
        assert np.array_equal(x[jj, tt], s1, equal_nan=True)
        assert np.array_equal(a[jj, tt], a1) and np.array_equal(r[jj, tt], r1)
        assert not ibits(x[~live]).any() and not ibits(a[~live]).any() and not ibits(r[~live]).any()   # +0.0 behind length


@pytest.mark.parametrize("shape", SHAPES, ids=[f"N{s[0]}-W{s[1]}-F{s[2]}" for s in SHAPES])
def test_gpu_per_env_with_identical_columns_is_the_lockstep_replay(shape):
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay
    N, W, F = shape
    B, H = 5, 4 * W + 9
    lengths = [W + 3, 1, 2 * W + 4, W + 1, 3 * W]                             # rows per episode; the ring wraps
    assert sum(lengths) > H
    bars = (100 * np.exp(0.01 * np.random.default_rng(N).standard_normal((sum(lengths), N, F - 1)).cumsum(0))).astype(np.float32)
    ms = MarketSeries(bars, device=DEV)
    lock = DeviceReplay(B, N, W, H, ms, features=F)
    per = DeviceReplay(B, N, W, H, ms, features=F, per_env=True)
    g = torch.Generator(device=DEV).manual_seed(N)
    t = 0
    for length in lengths:
        lock.new_episode()
        for k in range(length):
            day = torch.full((B,), t - 2, dtype=torch.int32, device=DEV)
            a, r = torch.rand(B, N, device=DEV, generator=g), torch.randn(B, device=DEV, generator=g)
            lock.add(day, a, r)
            per.add(day, a, r, done=torch.full((B,), int(k == length - 1), dtype=torch.uint8, device=DEV))
            t += 1
    assert per.count == lock.count == H and per.head == lock.head
    h0, env = lock.indices(S_MAX, generator=torch.Generator().manual_seed(2))
    for n in (1, 2, W + 1, 2 * W + 3):
        for u, v in zip(lock.gather_nstep(h0, env, n, GAMMA), per.gather_nstep(h0, env, n, GAMMA)):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    for L in (1, 3, W + 2):
        for tm in (True, False):
            for u, v in zip(lock.gather_sequences(h0, env, L, tm), per.gather_sequences(h0, env, L, tm)):
                assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    # new_episode() in per-env mode opens an episode for every env
    before = per._cur.clone()
    per.new_episode()
    assert torch.equal(per._cur, before + 1)


@pytest.mark.parametrize("B", [3, 70])
def test_gpu_priority_tree_per_env_tracks_the_valid_pairs(B):
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay, valid_pairs
    N, W = 4, 4
    H = 4 * W + 9
    rows = 3 * H
    bars = np.random.default_rng(0).standard_normal((rows + 8, N, 4)).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV), per_env=True, prioritized=True)
    done = done_rows(rows, B, W, seed=B)
    done_dev = torch.as_tensor(done.astype(np.uint8), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(B)
    L = H * B
    seen_open = seen_masked = False
    then = None
    for t in range(rows):
        rb.add(torch.full((B,), t, dtype=torch.int32, device=DEV), torch.rand(B, N, device=DEV, generator=g),
               torch.randn(B, device=DEV, generator=g), done=done_dev[t])
        ep, head, count = record(done[:t + 1], H)
        oldest = (head - count) % H
        pairs = valid_pairs(ep, oldest, count, W + 1, H)
        want = np.sort(((oldest + pairs[:, 0]) % H) * B + pairs[:, 1])
        _, lv = prio_ref.read_tree(rb.tree, L)
        assert np.array_equal(np.flatnonzero(lv[0] > 0), want), t
        prio_ref.check_levels(lv)
        seen_open |= len(want) > 0
        seen_masked |= 0 < len(want) and count - W - 1 > 0 and len(want) < (count - W - 1) * B
        if t == H + 3:                                                        # leaves sampled now, closed by later adds
            h0, env, leaf, w = rb.prioritized_indices(32, u=torch.linspace(0, 0.999, 32, dtype=torch.float64))
            assert set(leaf.cpu().numpy().tolist()) <= set(want.tolist())
            then = want.copy()
    assert seen_open and seen_masked
    ep, head, count = record(done, H)
    oldest = (head - count) % H
    pairs = valid_pairs(ep, oldest, count, W + 1, H)
    valid = set(map(tuple, pairs.tolist()))
    out = rb.sample_prioritized(64, generator=torch.Generator().manual_seed(1))
    h0, env = out[4] // B, out[4] % B
    got = set(zip(((h0.cpu().numpy().astype(np.int64) - oldest) % H).tolist(), env.cpu().numpy().tolist()))
    assert got <= valid and out[0].shape == (64, N, W, 5)
    # update_priorities on a since-closed leaf leaves it closed: the leaves open at add H + 3, some closed by now
    _, lv0 = prio_ref.read_tree(rb.tree, L)
    closed = np.setdiff1d(then, np.flatnonzero(lv0[0] > 0))
    assert closed.size > 0 and np.intersect1d(then, np.flatnonzero(lv0[0] > 0)).size > 0
    rb.update_priorities(torch.as_tensor(then, dtype=torch.int32), torch.full((then.size,), 3.0))
    _, lv1 = prio_ref.read_tree(rb.tree, L)
    assert not lv1[0][closed].any()
    assert np.array_equal(np.flatnonzero(lv1[0] > 0), np.flatnonzero(lv0[0] > 0))
    assert not np.array_equal(lv1[0], lv0[0])                                 # the open ones took the new value
    prio_ref.check_levels(lv1)


def test_gpu_off_policy_episodes_end_to_end():
    from pmenv import MarketSeries, TradingEnv
    from pmenv.episodes import Episodes
    from pmenv.off_policy import OffPolicy
    B, N, W, T, H = 8, 4, 4, 64, 40
    bars = (100 * np.exp(0.01 * np.random.default_rng(8).standard_normal((T, N, 4)).cumsum(0))).astype(np.float32)
    ms = MarketSeries(bars, device=DEV)
    env = TradingEnv(num_envs=B, num_assets=N, window=W, device=DEV, track_info=False)
    length = np.array([6, 7, 8, 9, 10, 11, 12, 6])
    start = 3 * np.arange(B)
    seen = []
    loop = OffPolicy(env, ms, capacity=H, update=lambda *a: seen.append(a), batch_size=64, episodes=True,
                     generator=torch.Generator().manual_seed(4))
    assert loop.replay.per_env
    ep = Episodes(ms, W, start, length=length)
    obs = ms.initial_window(ep.start, W)
    env.reset(obs)
    dones = []
    for _ in range(3):
        r, d = loop.collect_episodes(ep, obs, 12, random=True)
        assert r.shape == (12, B) and d.shape == (12, B) and d.dtype == torch.bool
        dones.append(d)
    dones = torch.cat(dones).cpu().numpy()                                    # [36, B]: ring row t is step t (36 < H)
    rb = loop.replay
    assert rb.count == 36 and rb.head == 36
    assert dones.any(0).all() and all(dones[:, b].sum() == 36 // length[b] for b in range(B))
    assert np.array_equal(rb.env_episode.cpu().numpy()[:36], np.concatenate([np.zeros((1, B), int), dones[:-1].cumsum(0)]))
    days = rb.days.cpu().numpy()

    def one_episode(h0, env_i, rows):                                         # rows h0 .. h0 + rows - 1 hold no done
        return all(not dones[h:h + k, b].any() for h, b, k in zip(h0, env_i, rows))

    def market_ok(s, h0, env_i):
        for j, (h, b) in enumerate(zip(h0, env_i)):
            d = days[h + W - 1, b]
            assert 0 <= d - (W - 1) and d < T
            assert np.array_equal(s[j, :, :, :4], bars[d - (W - 1):d + 1].transpose(1, 0, 2))
    g = torch.Generator().manual_seed(7)
    h0, e = rb.indices(64, generator=g)
    h0n, en = h0.cpu().numpy(), e.cpu().numpy()
    assert one_episode(h0n, en, [W] * 64)
    s, a, r, s2 = rb.gather(h0, e)
    market_ok(s.cpu().numpy(), h0n, en)
    out = rb.gather_nstep(h0, e, 3, GAMMA)
    m = out[4].cpu().numpy()
    assert one_episode(h0n, en, W + m - 1) and set(m.tolist()) <= {1, 2, 3} and len(set(m.tolist())) > 1
    market_ok(out[0].cpu().numpy(), h0n, en)
    h0, e = rb.sequence_indices(64, 3, generator=g)
    h0n, en = h0.cpu().numpy(), e.cpu().numpy()
    assert one_episode(h0n, en, [W + 3 - 1] * 64)
    x, _, _, ln = rb.gather_sequences(h0, e, 3)
    assert (ln == 3).all()
    market_ok(x[0].cpu().numpy(), h0n, en)
    # the loop's own sampling calls go through the same draws
    loop.update(1)
    assert len(seen) == 1 and seen[0][0].shape == (64, N, W, 5)
    for kw, n_args in ((dict(n_step=3), 5), (dict(seq_len=3), 3)):
        env2 = TradingEnv(num_envs=B, num_assets=N, window=W, device=DEV, track_info=False)
        got = []
        lp = OffPolicy(env2, ms, capacity=H, update=lambda *a: got.append(a), batch_size=16, episodes=True, **kw)
        ep2 = Episodes(ms, W, start, length=length)
        obs2 = ms.initial_window(ep2.start, W)
        env2.reset(obs2)
        lp.collect_episodes(ep2, obs2, 20)
        lp.update(1)
        assert len(got) == 1 and len(got[0]) == n_args
    lock = OffPolicy(env, ms, capacity=H)
    with pytest.raises(ValueError, match="episodes=True"):
        lock.collect_episodes(ep, obs, 1)
    with pytest.raises(ValueError, match="per_env"):
        lock.replay.add(torch.zeros(B, dtype=torch.int32, device=DEV), torch.rand(B, N, device=DEV),
                        torch.randn(B, device=DEV), done=torch.zeros(B, dtype=torch.uint8, device=DEV))
