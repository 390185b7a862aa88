"""n-step return samples of the device replay (pmenv_replay_gather_nstep) on an MI355X:
agent/td3/td3.py:85-106's fold done at sample time, against the one-step restatement of
replay/buffer.py:39-79 (oracle.replay_gather) composed with numpy. Needs a GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 3
GAMMA = 0.9


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


#          N,  W, F, S
SHAPES = [(4, 4, 5, 700),      # F = 5 persistent form, several samples per workgroup
          (30, 50, 5, 64),     # the product's whole-sample group (R = 30)
          (3, 3, 3, 64),       # 27 floats per sample: scalar write-out of the LDS form
          (8, 10, 8, 64),      # generic LDS form
          (300, 4, 5, 64),     # N > 256
          (257, 3, 5, 64)]     # N > 256 and no 16-B granular asset group: one thread per float
# the kernel each shape takes (pmenv_replay_path, asserted before any value is compared): the
# start of its name and the asset rows per group; the one-step gather's differ by name only
FORMS = {(4, 4, 5): ("replay_nstep_f5p_kernel<2,2>", 4),
         (30, 50, 5): ("replay_nstep_f5p_kernel<", 30),
         (3, 3, 3): ("replay_nstep_lds_kernel", 0),
         (8, 10, 8): ("replay_nstep_lds_kernel", 0),
         (300, 4, 5): ("replay_nstep_f5p_kernel<", 150),
         (257, 3, 5): ("replay_nstep_kernel", 0)}


def assert_form(kind, N, W, F, n, S, form):
    from pmenv.replay import gather_path
    name, R = form
    path = gather_path(kind, N, W, F, n=n, S=S).split(" ")
    assert path[0].startswith(name) and path[1] == f"R={R}", path


@functools.lru_cache(maxsize=None)
def ring(N, W, F, S):
    """A wrapped ring of three episodes of unequal length — the oldest cut by the wrap to
    W + 3 rows, then 3W + 8 rows, then 2W + 3 — whose day indices run off both ends of the
    series, the sampled indices (hand-picked ones first, then seeded random ones) and the
    one-step restatement at those indices."""
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
    run = nstep_counts(rb._row_ep, oldest, rb.count, W, H, st, 10 ** 6)      # the fold's length with no cap
    days, actions, rewards = rb.days.cpu().numpy(), rb.actions.cpu().numpy(), rb.rewards.cpu().numpy()
    dl = days[(h0 + W - 1) % H, env]
    assert (dl - (W - 1) < 0).any() and (dl + 1 >= T).any()                 # windows off both ends of the series
    one = replay_gather(bars, days, actions, rewards, h0, env, W)
    return dict(rb=rb, bars=bars, H=H, oldest=oldest, span=span, st=st, run=run, days=days, actions=actions,
                rewards=rewards, h0=h0, env=env, one=one,
                h0_dev=torch.as_tensor(h0, device=DEV), env_dev=torch.as_tensor(env, device=DEV))


def n_values(W):
    return [1, 2, W - 1, W, W + 1, 2 * W + 3]


CASES = [(shape, k) for shape in SHAPES for k in range(6)]


@pytest.mark.parametrize("shape,k", CASES, ids=[f"N{s[0]}-W{s[1]}-F{s[2]}-n{n_values(s[1])[k]}" for s, k in CASES])
def test_gpu_replay_nstep_matches_composed_restatement(shape, k):
    from pmenv.replay import nstep_counts
    from oracle import replay_gather
    N, W, F, S = shape
    n = n_values(W)[k]
    c = ring(*shape)
    rb, H, h0, env, st, run = c["rb"], c["H"], c["h0"], c["env"], c["st"], c["run"]
    m = nstep_counts(rb._row_ep, c["oldest"], rb.count, W, H, st, n)
    # the drawn indices hold every way a fold can end (a condition on the inputs)
    assert n <= 2 * W + 8 and (m == n).any()                                 # episode 2 has 2W + 8 starts: a full fold
    assert ((m == run) & (st + m < c["span"])).any()                         # stopped by an episode boundary
    assert ((m == run) & (st + m == c["span"])).any()                        # stopped by the newest rows
    assert n == 1 or ((m < n) & (st + m < c["span"])).any() and ((m < n) & (st + m == c["span"])).any()
    es, ea, er1, _ = c["one"]
    _, _, _, es2 = replay_gather(c["bars"], c["days"], c["actions"], c["rewards"], (h0 + m - 1) % H, env, W)
    g64 = np.float64(np.float32(GAMMA))
    eR = np.empty(S, np.float64)
    ed = np.empty(S, np.float64)
    for j in range(S):
        r = c["rewards"][(h0[j] + W - 1 + np.arange(m[j])) % H, env[j]].astype(np.float64)
        acc = r[-1]
        for x in r[-2::-1]:                                                  # td3.py:94-96
            acc = x + g64 * acc
        eR[j] = acc
        ed[j] = np.prod(np.full(m[j], g64))
    assert_form("nstep", N, W, F, n, S, FORMS[N, W, F])
    s, a, R, s2, steps, disc = rb.gather_nstep(c["h0_dev"], c["env_dev"], n, GAMMA)
    assert s.shape == (S, N, W, F) and s2.shape == s.shape and a.shape == (S, N, 1) and R.shape == (S, 1, 1)
    assert steps.shape == (S,) and steps.dtype == torch.int32 and disc.shape == (S,)
    assert np.array_equal(steps.cpu().numpy(), m)
    assert np.array_equal(s.cpu().numpy(), es, equal_nan=True)
    assert np.array_equal(s2.cpu().numpy(), es2, equal_nan=True)
    assert np.array_equal(a.cpu().numpy()[..., 0], ea)
    R, disc = R.cpu().numpy()[:, 0, 0].astype(np.float64), disc.cpu().numpy().astype(np.float64)
    assert (np.abs(R - eR) <= 1e-6 * np.abs(eR) + 1e-9).all()
    assert (np.abs(disc - ed) <= 1e-6 * np.abs(ed) + 1e-9).all()
    if n == 1:                                                               # the one-step gather, bit for bit
        name, rows = FORMS[N, W, F]
        assert_form("one_step", N, W, F, 1, S, (name.replace("nstep", "gather"), rows))
        s1, a1, r1, s21 = rb.gather(c["h0_dev"], c["env_dev"])
        out = rb.gather_nstep(c["h0_dev"], c["env_dev"], 1, GAMMA)
        for x, y in zip(out[:4], (s1, a1, r1, s21)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert np.array_equal(r1.cpu().numpy()[:, 0, 0], er1) and (out[4] == 1).all()


def test_gpu_replay_nstep_days_that_skip_take_the_two_pass_path():
    """Day indices that do not advance by one a row (a caller's own ring): s' still ends at
    days[h0+m+W-2] + 1, whatever the distance to s."""
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay
    from oracle import replay_gather
    N, W, H, T, n = 4, 4, 40, 60, 3
    rng = np.random.default_rng(2)
    bars = rng.standard_normal((T, N, 4)).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV))
    for k in range(H - 6):
        rb.add(torch.full((B,), (7 * k) % T, dtype=torch.int32, device=DEV), torch.rand(B, N, device=DEV),
               torch.randn(B, device=DEV))
    S = rb.count - W - 1                                                     # every start, oldest = row 0
    h0 = torch.arange(S, dtype=torch.int32, device=DEV)
    env = h0 % B
    s, a, R, s2, steps, disc = rb.gather_nstep(h0, env, n, GAMMA)
    m = steps.cpu().numpy()
    assert np.array_equal(m, np.minimum(n, S - np.arange(S)))
    d, ac, rw = rb.days.cpu().numpy(), rb.actions.cpu().numpy(), rb.rewards.cpu().numpy()
    es, ea, _, _ = replay_gather(bars, d, ac, rw, h0.cpu().numpy(), env.cpu().numpy(), W)
    _, _, _, es2 = replay_gather(bars, d, ac, rw, (h0.cpu().numpy() + m - 1) % H, env.cpu().numpy(), W)
    assert np.array_equal(s.cpu().numpy(), es, equal_nan=True) and np.array_equal(s2.cpu().numpy(), es2, equal_nan=True)
    assert np.array_equal(a.cpu().numpy()[..., 0], ea)


def test_gpu_replay_nstep_argument_errors():
    from pmenv import _abi
    c = ring(*SHAPES[0])
    rb, (N, W, F, S) = c["rb"], SHAPES[0]
    lib = _abi.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s = torch.zeros(S, N, W, F, device=DEV)
    s2, a, r = torch.zeros_like(s), torch.zeros(S, N, device=DEV), torch.zeros(S, device=DEV)
    steps, disc = torch.full((S,), -7, dtype=torch.int32, device=DEV), torch.zeros(S, device=DEV)

    def call(n=2, gamma=GAMMA, count=rb.count, steps_p=P(steps)):
        return lib.pmenv_replay_gather_nstep(P(rb.series.bars), rb.series.bars.shape[0], N, F, W, P(rb.days),
                                             P(rb.actions), P(rb.rewards), rb.H, B, P(c["h0_dev"]), P(c["env_dev"]),
                                             S, P(rb._row_ep_dev), c["oldest"], count, n, gamma, P(s), P(s2), P(a),
                                             P(r), steps_p, P(disc), None)
    rb.gather_nstep(c["h0_dev"], c["env_dev"], 2, GAMMA)                     # the episode ids are on the device
    assert call(n=0) == -1 and call(gamma=0.0) == -1 and call(gamma=1.5) == -1 and call(gamma=float("nan")) == -1
    assert call(count=rb.H + 1) == -1 and call(steps_p=None) == -1
    torch.cuda.synchronize()
    assert (steps == -7).all() and not s.any() and not s2.any()              # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert (steps >= 1).all() and (steps <= 2).all()


def test_gpu_off_policy_nstep_update_gets_five_tensors():
    from pmenv import MarketSeries, TradingEnv
    from pmenv.off_policy import OffPolicy
    Bn, N, W, T = 16, 7, 6, 200
    rng = np.random.default_rng(3)
    bars = (100 * np.exp(0.01 * rng.standard_normal((T, N, 4)).cumsum(0))).astype(np.float32)
    m = MarketSeries(bars, device=DEV)
    env = TradingEnv(num_envs=Bn, num_assets=N, window=W, device=DEV)
    seen = []
    loop = OffPolicy(env, m, capacity=40, update=lambda *args: seen.append(args), batch_size=64,
                     generator=torch.Generator().manual_seed(3), n_step=3, gamma=GAMMA)
    g = torch.Generator().manual_seed(5)
    loop.collect(m.random_starts(Bn, W, 12, generator=g), 12)
    loop.collect(m.random_starts(Bn, W, 14, generator=g), 14)                # a second episode in the ring
    loop.update(1)
    assert len(seen) == 1 and len(seen[0]) == 5
    s, a, R, s_, disc = seen[0]
    assert s.shape == (64, N, W, 5) and s_.shape == s.shape and a.shape == (64, N, 1) and R.shape == (64, 1, 1)
    g64 = np.float64(np.float32(GAMMA))
    table = torch.tensor([np.float32(np.prod(np.full(k, g64))) for k in range(4)], device=DEV)   # gamma ** steps
    assert disc.shape == (64,) and torch.isin(disc, table[1:]).all()
    out = loop.replay.sample_nstep(256, 3, GAMMA, generator=torch.Generator().manual_seed(9))
    steps, disc = out[4], out[5]
    assert int(steps.min()) >= 1 and int(steps.max()) <= 3 and len(steps.unique()) == 3
    assert torch.equal(disc, table[steps.long()])


def test_gpu_off_policy_default_update_keeps_four_tensors():
    from pmenv import MarketSeries, TradingEnv
    from pmenv.off_policy import OffPolicy
    Bn, N, W, T = 16, 7, 6, 200
    bars = (100 * np.exp(0.01 * np.random.default_rng(4).standard_normal((T, N, 4)).cumsum(0))).astype(np.float32)
    m = MarketSeries(bars, device=DEV)
    env = TradingEnv(num_envs=Bn, num_assets=N, window=W, device=DEV)
    seen = []
    loop = OffPolicy(env, m, capacity=40, update=lambda *args: seen.append(args), batch_size=32)
    assert loop.n_step == 1 and loop.gamma == 0.997
    loop.collect(m.random_starts(Bn, W, 12, generator=torch.Generator().manual_seed(5)), 12)
    loop.update(1)
    assert len(seen) == 1 and len(seen[0]) == 4 and seen[0][2].shape == (32, 1, 1)
