"""Sequence samples of the device replay (pmenv_replay_gather_seq) on an MI355X: element t
of sequence j is the one-step sample at start h0[j] + t, against the one-step restatement
of replay/buffer.py:39-79 (oracle.replay_gather) called once per element. Needs a GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


#          N,  W, F, S
SHAPES = [(4, 4, 5, 200),      # fast form, many items per workgroup
          (30, 50, 5, 16),     # the product's whole-sample group (R = 30)
          (3, 3, 3, 16),       # generic form
          (8, 10, 8, 16),      # generic form
          (300, 4, 5, 16)]     # N > 256
# the kernel each shape takes (pmenv_replay_path, asserted before any value is compared): the
# start of its name and the asset rows per group
FORMS = {(4, 4, 5): ("replay_seq_f5p_kernel<2,16>", 4),
         (30, 50, 5): ("replay_seq_f5p_kernel<", 30),
         (3, 3, 3): ("replay_seq_kernel", 0),
         (8, 10, 8): ("replay_seq_kernel", 0),
         (300, 4, 5): ("replay_seq_f5p_kernel<", 150)}


def l_values(W):
    return [1, 2, W, W + 1, 2 * W + 3]


@functools.lru_cache(maxsize=None)
def ring(N, W, F, S):
    """A wrapped ring of three episodes of unequal length — the oldest cut by the wrap to
    W + 3 rows, then 3W + 8 rows, then 2W + 3 — whose day indices run off both ends of the
    series; the sampled starts (hand-picked ones first, then seeded random ones); and the
    one-step restatement of every element a sequence of up to 2W + 3 elements can hold:
    ex / ea / er [S, Lmax, ..], filled for t < run[j] and zero behind (computed once)."""
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay, nstep_counts
    from oracle import replay_gather
    e2, e3 = 3 * W + 8, 2 * W + 3
    H = (W + 3) + e2 + e3
    e1 = H - 5
    T = 4 * W + 12
    rng = np.random.default_rng(N * 100 + W)
    bars = (100 * np.exp(0.01 * rng.standard_normal((T, N, F - 1)).cumsum(0))).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV), features=F)
    g = torch.Generator(device=DEV).manual_seed(N + W)
    env_off = torch.arange(B, dtype=torch.int32, device=DEV)
    # first recorded day per episode: the kept rows of episode 1 start 3 days before the
    # series, episode 3 ends 4 days past it
    for length, day0 in ((e1, -3 - (e1 - (W + 3))), (e2, W), (e3, T + 4 - e3 - (B - 1))):
        rb.new_episode()
        for k in range(length):
            rb.add(day0 + k + env_off, torch.rand(B, N, device=DEV, generator=g),
                   torch.randn(B, device=DEV, generator=g))
    oldest = (rb.head - rb.count) % H
    assert rb.count == H and e1 + e2 + e3 > H and rb.head == oldest > 0      # wrapped: the oldest row is mid-array
    span = H - W - 1
    first2, last2 = W + 3, W + 3 + e2 - W - 1                                # episode 2's first / last valid start
    picked = [first2, first2 + 1, last2, last2 - 1, last2 - 2, span - 1, span - 2, span - 3, 0, 1]
    h0r, envr = rb.indices(S - len(picked), generator=torch.Generator().manual_seed(N))
    st = np.concatenate([np.array(picked), (h0r.cpu().numpy().astype(np.int64) - oldest) % H])
    env = np.concatenate([np.arange(len(picked)) % B, envr.cpu().numpy()]).astype(np.int32)
    h0 = ((oldest + st) % H).astype(np.int32)
    run = nstep_counts(rb._row_ep, oldest, rb.count, W, H, st, 10 ** 6)      # a sequence's length with no cap
    days, actions, rewards = rb.days.cpu().numpy(), rb.actions.cpu().numpy(), rb.rewards.cpu().numpy()
    Lmax = l_values(W)[-1]
    jj, tt = np.nonzero(np.arange(Lmax)[None, :] < run[:, None])            # every element of every sequence
    s1, a1, r1, _ = replay_gather(bars, days, actions, rewards, (h0[jj] + tt) % H, env[jj], W)
    ex = np.zeros((S, Lmax, N, W, F), np.float32)
    ea = np.zeros((S, Lmax, N), np.float32)
    er = np.zeros((S, Lmax), np.float32)
    ex[jj, tt], ea[jj, tt], er[jj, tt] = s1, a1, r1
    dl = days[(h0[:, None] + np.arange(Lmax)[None, :] + W - 1) % H, env[:, None]]   # [S, Lmax] last day of element t
    return dict(rb=rb, H=H, oldest=oldest, span=span, st=st, run=run, h0=h0, env=env, ex=ex, ea=ea, er=er, dl=dl, T=T,
                h0_dev=torch.as_tensor(h0, device=DEV), env_dev=torch.as_tensor(env, device=DEV))


CASES = [(shape, k, tm) for shape in SHAPES for k in range(5) for tm in (True, False)]


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


@pytest.mark.parametrize("shape,k,time_major", CASES,
                         ids=[f"N{s[0]}-W{s[1]}-F{s[2]}-L{l_values(s[1])[k]}-{'tm' if tm else 'bm'}"
                              for s, k, tm in CASES])
def test_gpu_replay_seq_matches_one_step_restatement(shape, k, time_major):
    from pmenv.replay import nstep_counts
    N, W, F, S = shape
    L = l_values(W)[k]
    c = ring(*shape)
    rb, st, run, span = c["rb"], c["st"], c["run"], c["span"]
    m = nstep_counts(rb._row_ep, c["oldest"], rb.count, W, c["H"], st, L)
    live = np.arange(L)[None, :] < m[:, None]                                # [S, L]
    # the drawn starts hold every way a sequence can end (conditions on the inputs). L = 1
    # cannot be cut short: m >= 1 = L for every valid start
    assert L <= 2 * W + 8 and (m == L).any()                                 # episode 2 has 2W + 8 starts: a full one
    if L > 1:
        assert ((m < L) & (st + m < span)).any()                             # cut by an episode boundary
        assert ((m < L) & (st + m == span)).any()                            # cut by the newest rows
    dl = c["dl"][:, :L]
    assert (live & (dl - (W - 1) < 0)).any() and (live & (dl >= c["T"])).any()   # windows off both ends of the series
    ex, ea, er = c["ex"][:, :L].copy(), c["ea"][:, :L].copy(), c["er"][:, :L].copy()
    ex[~live], ea[~live], er[~live] = 0.0, 0.0, 0.0                          # the table holds elements up to run >= m
    from pmenv.replay import gather_path
    path = gather_path("seq", N, W, F, n=L, S=S).split(" ")
    assert path[0].startswith(FORMS[N, W, F][0]) and path[1] == f"R={FORMS[N, W, F][1]}", path
    x, a, r, length = rb.gather_sequences(c["h0_dev"], c["env_dev"], L, time_major=time_major)
    lead = (L, S) if time_major else (S, L)
    assert x.shape == lead + (N, W, F) and a.shape == lead + (N,) and r.shape == lead
    assert x.dtype == a.dtype == r.dtype == torch.float32
    assert length.shape == (S,) and length.dtype == torch.int32
    assert np.array_equal(length.cpu().numpy(), m)
    x, a, r = x.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy()
    if time_major:
        x, a, r = x.swapaxes(0, 1), a.swapaxes(0, 1), r.swapaxes(0, 1)
    assert np.array_equal(x[live], ex[live], equal_nan=True)
    assert np.array_equal(a[live], ea[live]) and np.array_equal(r[live], er[live])
    assert not bits(x[~live]).any() and not bits(a[~live]).any() and not bits(r[~live]).any()   # +0.0 bits


@pytest.mark.parametrize("shape", SHAPES, ids=[f"N{s[0]}-W{s[1]}-F{s[2]}" for s in SHAPES])
def test_gpu_replay_seq_layouts_are_permutations(shape):
    N, W, F, S = shape
    c = ring(*shape)
    for L in (2, W + 1):
        tm = c["rb"].gather_sequences(c["h0_dev"], c["env_dev"], L, time_major=True)
        bm = c["rb"].gather_sequences(c["h0_dev"], c["env_dev"], L, time_major=False)
        for u, v in zip(tm[:3], bm[:3]):
            assert torch.equal(u.transpose(0, 1).contiguous().view(torch.int32), v.view(torch.int32))
        assert torch.equal(tm[3], bm[3])


@pytest.mark.parametrize("shape", SHAPES, ids=[f"N{s[0]}-W{s[1]}-F{s[2]}" for s in SHAPES])
def test_gpu_replay_seq_of_one_is_the_one_step_gather(shape):
    N, W, F, S = shape
    c = ring(*shape)
    s, a1, r1, _ = c["rb"].gather(c["h0_dev"], c["env_dev"])
    for time_major in (True, False):
        x, a, r, length = c["rb"].gather_sequences(c["h0_dev"], c["env_dev"], 1, time_major=time_major)
        assert torch.equal(x.reshape(S, N, W, F).view(torch.int32), s.view(torch.int32))
        assert torch.equal(a.reshape(S, N).view(torch.int32), a1.reshape(S, N).view(torch.int32))
        assert torch.equal(r.reshape(S).view(torch.int32), r1.reshape(S).view(torch.int32))
        assert (length == 1).all()


def test_gpu_replay_seq_long_chunks():
    """Enough sequences that the chunks are full size (the short batches above are split
    into smaller ones so that every CU gets work): 1,100 sequences of 40 elements from one
    episode, against the one-step gather at every element's start."""
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay
    N, W, H, T, L, S = 4, 4, 64, 80, 40, 1100
    bars = np.random.default_rng(7).standard_normal((T, N, 4)).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV))
    g = torch.Generator(device=DEV).manual_seed(7)
    for k in range(H - 4):                                                   # days run off the end of the series
        rb.add(torch.full((B,), 30 + k, dtype=torch.int32, device=DEV), torch.rand(B, N, device=DEV, generator=g),
               torch.randn(B, device=DEV, generator=g))
    span = rb.count - W - 1
    h0 = torch.arange(S, dtype=torch.int32, device=DEV) % span               # every start, short tails included
    env = torch.arange(S, dtype=torch.int32, device=DEV) % B
    x, a, r, length = rb.gather_sequences(h0, env, L, time_major=False)
    m = torch.minimum(torch.tensor(L, device=DEV), span - h0).to(torch.int32)
    assert torch.equal(length, m) and int(m.min()) == 1 and int(m.max()) == L
    tt = torch.arange(L, dtype=torch.int32, device=DEV)
    live = tt[None, :] < m[:, None]
    jj, tl = torch.nonzero(live, as_tuple=True)
    s1, a1, r1, _ = rb.gather((h0[jj] + tl.to(torch.int32)) % H, env[jj])
    assert torch.isnan(s1).any()
    assert torch.equal(x[jj, tl].view(torch.int32), s1.view(torch.int32))
    assert torch.equal(a[jj, tl].view(torch.int32), a1[..., 0].view(torch.int32))
    assert torch.equal(r[jj, tl].view(torch.int32), r1[:, 0, 0].view(torch.int32))
    assert not x[~live].view(torch.int32).any() and not a[~live].view(torch.int32).any()
    assert not r[~live].view(torch.int32).any()


@pytest.mark.parametrize("F", [5, 3])
def test_gpu_replay_seq_days_that_skip(F):
    """Day indices that do not advance by one a row (a caller's own ring): each element is
    still its own one-step s, the window ending at days[h0+t+W-1]."""
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay
    from oracle import replay_gather
    N, W, H, T, L = 4, 4, 40, 60, 5
    rng = np.random.default_rng(2)
    bars = rng.standard_normal((T, N, F - 1)).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV), features=F)
    for k in range(H - 6):
        rb.add(torch.full((B,), (7 * k) % T, dtype=torch.int32, device=DEV), torch.rand(B, N, device=DEV),
               torch.randn(B, device=DEV))
    rb.days[12:22] = (20 + torch.arange(10, dtype=torch.int32, device=DEV))[:, None]   # a run of unit steps inside
    span = rb.count - W - 1                                                  # oldest = row 0
    S = 1100                                                                 # enough that a chunk is the whole sequence
    h0 = torch.arange(S, dtype=torch.int32, device=DEV) % span               # every start, many times
    env = torch.arange(S, dtype=torch.int32, device=DEV) % B
    x, a, r, length = rb.gather_sequences(h0, env, L, time_major=False)
    m = length.cpu().numpy()
    assert np.array_equal(m, np.minimum(L, span - h0.cpu().numpy()))
    d, ac, rw = rb.days.cpu().numpy(), rb.actions.cpu().numpy(), rb.rewards.cpu().numpy()
    x, a, r = x.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy()
    h0n, envn = h0.cpu().numpy(), env.cpu().numpy()
    for t in range(L):
        ok = t < m
        es, ea, er, _ = replay_gather(bars, d, ac, rw, (h0n[ok] + t) % H, envn[ok], W)
        assert np.array_equal(x[ok, t], es, equal_nan=True)
        assert np.array_equal(a[ok, t], ea) and np.array_equal(r[ok, t], er)
        assert not bits(x[~ok, t]).any() and not bits(a[~ok, t]).any() and not bits(r[~ok, t]).any()


def test_gpu_replay_sample_sequences_are_full_length():
    c = ring(*SHAPES[0])
    rb, (N, W, F, _) = c["rb"], SHAPES[0]
    L, S = W + 1, 64
    for time_major in (True, False):
        x, a, r, length = rb.sample_sequences(S, L, generator=torch.Generator().manual_seed(4), time_major=time_major)
        lead = (L, S) if time_major else (S, L)
        assert x.shape == lead + (N, W, F) and a.shape == lead + (N,) and r.shape == lead
        assert x.dtype == a.dtype == r.dtype == torch.float32 and length.dtype == torch.int32
        assert length.shape == (S,) and (length == L).all()
    h0, env = rb.sequence_indices(256, L, generator=torch.Generator().manual_seed(5))
    assert h0.dtype == env.dtype == torch.int32 and h0.device == rb.days.device
    st = (h0.cpu().numpy().astype(np.int64) - c["oldest"]) % c["H"]
    from pmenv.replay import sequence_starts
    table = sequence_starts(rb._row_ep, c["oldest"], rb.count, W, c["H"], L)
    assert np.isin(st, table).all() and len(np.unique(st)) > 1 and len(np.unique(env.cpu().numpy())) == B
    key = rb._seq_key
    rb.sequence_indices(8, L)                                                # the table is cached per (ring state, L)
    assert rb._seq_key == key and key[-1] == L
    rb.sequence_indices(8, L - 1)
    assert rb._seq_key != key


def test_gpu_replay_sequence_indices_raise_without_a_run_of_l():
    c = ring(*SHAPES[0])
    rb, W = c["rb"], SHAPES[0][1]
    rb.sequence_indices(4, 2 * W + 8)                                        # episode 2 holds exactly one such start
    with pytest.raises(ValueError):
        rb.sequence_indices(4, 2 * W + 9)
    with pytest.raises(ValueError):
        rb.sequence_indices(4, rb.count)                                     # longer than the ring
    with pytest.raises(ValueError):
        rb.sequence_indices(4, 0)


def test_gpu_replay_seq_argument_errors():
    from pmenv import _abi
    c = ring(*SHAPES[0])
    rb, (N, W, F, S) = c["rb"], SHAPES[0]
    lib = _abi.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    L = 3
    x = torch.zeros(S, L, N, W, F, device=DEV)
    a, r = torch.zeros(S, L, N, device=DEV), torch.zeros(S, L, device=DEV)
    length = torch.full((S,), -7, dtype=torch.int32, device=DEV)

    def call(L=L, count=rb.count, oldest=c["oldest"], x_p=P(x), len_p=P(length), ep_p=P(rb._row_ep_dev), H=rb.H,
             S=S, F=F):
        return lib.pmenv_replay_gather_seq(P(rb.series.bars), rb.series.bars.shape[0], N, F, W, P(rb.days),
                                           P(rb.actions), P(rb.rewards), H, B, P(c["h0_dev"]), P(c["env_dev"]), S,
                                           ep_p, oldest, count, L, 0, x_p, P(a), P(r), len_p, None)
    rb.gather_sequences(c["h0_dev"], c["env_dev"], 2)                        # the episode ids are on the device
    assert call(L=0) == -1 and call(L=-3) == -1
    assert call(count=rb.H + 1) == -1 and call(count=-1) == -1
    assert call(oldest=-1) == -1 and call(oldest=rb.H) == -1
    assert call(x_p=None) == -1 and call(len_p=None) == -1
    assert call(H=W) == -1 and call(S=0) == -1 and call(F=1) == -1           # the n-step entry's shape errors
    torch.cuda.synchronize()
    assert (length == -7).all() and not x.any() and not a.any() and not r.any()   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert (length >= 1).all() and (length <= L).all() and x.any()


def _loop(seen, **kw):
    from pmenv import MarketSeries, TradingEnv
    from pmenv.off_policy import OffPolicy
    Bn, N, W, T = 16, 7, 6, 200
    rng = np.random.default_rng(3)
    bars = (100 * np.exp(0.01 * rng.standard_normal((T, N, 4)).cumsum(0))).astype(np.float32)
    m = MarketSeries(bars, device=DEV)
    env = TradingEnv(num_envs=Bn, num_assets=N, window=W, device=DEV)
    return m, OffPolicy(env, m, capacity=40, update=lambda *args: seen.append(args), batch_size=32,
                        generator=torch.Generator().manual_seed(3), **kw)


def test_gpu_off_policy_seq_len_update_gets_time_major_sequences():
    seen = []
    m, loop = _loop(seen, seq_len=8)
    g = torch.Generator().manual_seed(5)
    loop.collect(m.random_starts(16, 6, 16, generator=g), 16)
    loop.collect(m.random_starts(16, 6, 18, generator=g), 18)                # a second episode in the ring
    loop.update(2)
    assert len(seen) == 2 and len(seen[0]) == 3
    x, a, r = seen[0]
    assert x.shape == (8, 32, 7, 6, 5) and a.shape == (8, 32, 7) and r.shape == (8, 32)
    assert torch.isfinite(x).all() and (a.sum(-1) - 1).abs().max() < 1e-5    # full sequences: every a a simplex point
    # element t + 1 is element t one step on: its weight channel drops the oldest action
    assert torch.equal(x[1:, :, :, :-1, 4], x[:-1, :, :, 1:, 4])


def test_gpu_off_policy_seq_len_with_n_step_raises():
    with pytest.raises(ValueError):
        _loop([], seq_len=8, n_step=3)
    seen = []
    _, loop = _loop(seen)
    assert loop.seq_len == 0 and loop.n_step == 1
