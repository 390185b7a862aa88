"""The priority tree of the device replay (pmenv_prio_*, include/pmenv.h) on an MI355X,
against the numpy f64 restatement of tests/prio_ref.py: the tree's shape, exact and
bracketed sampling, the importance weights, updates, the replay's leaf invariant, graph
capture and OffPolicy(prioritized=True). Needs a GPU."""
import functools

import numpy as np
import pytest
import torch

import prio_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(DEV)


def dev(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def make_tree(vals):
    """A tree whose leaves hold `vals` (f32, 0 or >= FLT_MIN), every node computed by the
    device: the live leaves are marked by hand, then one update with alpha = 1, eps = 0
    gives each its value and refreshes its ancestors."""
    from pmenv.replay import prio_tree, prio_update
    vals = np.asarray(vals, dtype=np.float32)
    L = len(vals)
    tree = prio_tree(L, DEV)
    tree[64:64 + 4 * L].view(torch.float32).copy_(dev((vals > 0).astype(np.float32), torch.float32))
    prio_update(tree, L, torch.arange(L, dtype=torch.int32, device=DEV), dev(vals, torch.float32), 1.0, 0.0)
    mx, lv = prio_ref.read_tree(tree, L)
    assert np.array_equal(lv[0], vals) and mx == max(1.0, vals.max())
    return tree


def sample(tree, L, u, beta=0.4, Bn=B):
    from pmenv.replay import prio_sample
    out = prio_sample(tree, L, Bn, dev(u, torch.float64), beta)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


# ---------------------------------------------------------------- tree shape
@pytest.mark.parametrize("L", [1, 63, 64, 65, 4096, 4097, 262145])
def test_gpu_prio_tree_shape_after_init_fill_update(L):
    from pmenv.replay import prio_fill, prio_tree, prio_update
    tree = prio_tree(L, DEV)
    mx, lv = prio_ref.read_tree(tree, L)
    assert mx == 1.0 and all(not x.view(np.uint8).any() for x in lv)          # init: all zero, maximum 1
    assert len(lv) == {1: 2, 63: 2, 64: 2, 65: 2, 4096: 2, 4097: 3, 262145: 4}[L]
    prio_fill(tree, L, None, 0, L)                                           # every leaf opens at the maximum
    mx, lv = prio_ref.read_tree(tree, L)
    assert mx == 1.0 and (lv[0] == 1.0).all()
    prio_ref.check_levels(lv)
    assert lv[-1].sum() == L                                                 # sums of ones are exact
    # an update of a random subset, duplicates included
    rng = np.random.default_rng(L)
    S = min(L, 300)
    idx = rng.integers(0, L, S).astype(np.int32)
    td = rng.standard_normal(S).astype(np.float32) * 3
    prio_update(tree, L, dev(idx, torch.int32), dev(td, torch.float32), 0.6, 1e-6)
    mx2, lv2 = prio_ref.read_tree(tree, L)
    prio_ref.check_levels(lv2)
    new = prio_ref.priority(td, 0.6, 1e-6, 1.0)
    assert np.allclose(mx2, max(1.0, new.max()), rtol=1e-6)
    want = lv[0].copy()
    for i in np.unique(idx):
        want[i] = new[idx == i].max()
    assert np.allclose(lv2[0], want, rtol=1e-6) and np.array_equal(lv2[0] == 1.0, want == 1.0)
    for k, touched in enumerate(prio_ref.ancestors(idx, len(lv) - 1), start=1):
        keep = np.ones(len(lv[k]), bool)
        keep[touched] = False
        assert np.array_equal(lv2[k][keep].view(np.int64), lv[k][keep].view(np.int64))   # untouched: the same bits
    # a fill that closes one run and opens another, both crossing node borders where L allows
    n = max(1, min(L // 4, 130))
    c0 = L // 3
    o0 = 2 * L // 3 if 2 * L // 3 >= c0 + n and 2 * L // 3 + n <= L else None
    prio_fill(tree, L, c0, o0, n)
    mx3, lv3 = prio_ref.read_tree(tree, L)
    prio_ref.check_levels(lv3)
    want = lv2[0].copy()
    want[c0:c0 + n] = 0.0
    touched = np.arange(c0, c0 + n)
    if o0 is not None:
        want[o0:o0 + n] = mx2
        touched = np.concatenate([touched, np.arange(o0, o0 + n)])
    assert mx3 == mx2 and np.array_equal(lv3[0].view(np.int32), want.view(np.int32))
    for k, t in enumerate(prio_ref.ancestors(touched, len(lv) - 1), start=1):
        keep = np.ones(len(lv[k]), bool)
        keep[t] = False
        assert np.array_equal(lv3[k][keep].view(np.int64), lv2[k][keep].view(np.int64))
    prio_fill(tree, L, 0, None, L)                                           # closing everything: an all-zero tree again
    _, lv4 = prio_ref.read_tree(tree, L)
    assert all(not x.view(np.uint8).any() for x in lv4)


def test_gpu_prio_argument_errors():
    from pmenv import _abi
    from pmenv.replay import prio_tree
    import ctypes
    lib = _abi.load()
    L = 130
    tree = prio_tree(L, DEV)
    before = tree.clone()
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    u = torch.zeros(4, dtype=torch.float64, device=DEV)
    i4 = [torch.full((4,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    w = torch.zeros(4, device=DEV)
    assert lib.pmenv_prio_init(None, L, None) == -1 and lib.pmenv_prio_init(P(tree), 0, None) == -1
    assert lib.pmenv_prio_init(P(tree), 2 ** 31, None) == -1
    assert lib.pmenv_prio_init(ctypes.c_void_p(tree.data_ptr() + 4), L, None) == -4
    assert lib.pmenv_prio_fill(P(tree), L, 100, -1, 31, None) == -1          # past the leaves
    assert lib.pmenv_prio_fill(P(tree), L, 0, 5, 10, None) == -1             # overlapping ranges
    assert lib.pmenv_prio_fill(P(tree), L, 0, 10, -1, None) == -1
    assert lib.pmenv_prio_fill(P(tree), L, -1, -1, 10, None) == 0 and lib.pmenv_prio_fill(P(tree), L, 0, 10, 0, None) == 0
    assert lib.pmenv_prio_sample(P(tree), L, 0, P(u), 4, 0.4, P(i4[0]), P(i4[1]), P(i4[2]), P(w), None) == -1
    assert lib.pmenv_prio_sample(P(tree), L, B, None, 4, 0.4, P(i4[0]), P(i4[1]), P(i4[2]), P(w), None) == -1
    assert lib.pmenv_prio_sample(P(tree), L, B, P(u), 0, 0.4, P(i4[0]), P(i4[1]), P(i4[2]), P(w), None) == -1
    assert lib.pmenv_prio_sample(P(tree), L, B, P(u), 4, -0.1, P(i4[0]), P(i4[1]), P(i4[2]), P(w), None) == -1
    assert lib.pmenv_prio_sample(P(tree), L, B, P(u), 4, 0.4, P(i4[0]), None, P(i4[2]), P(w), None) == -1
    assert lib.pmenv_prio_update(P(tree), L, P(i4[0]), None, 4, 0.6, 1e-6, None) == -1
    assert lib.pmenv_prio_update(P(tree), L, P(i4[0]), P(w), 4, -1.0, 1e-6, None) == -1
    assert lib.pmenv_prio_update(P(tree), L, P(i4[0]), P(w), 4, 0.6, float("nan"), None) == -1
    assert lib.pmenv_prio_update(P(tree), L, P(i4[0]), P(w), 0, 0.6, 1e-6, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(tree, before) and all((x == -7).all() for x in i4)    # nothing was launched
    # an empty tree samples leaf 0 with weight 0; indices outside the leaves are skipped by update
    assert lib.pmenv_prio_sample(P(tree), L, B, P(u), 4, 0.4, P(i4[0]), P(i4[1]), P(i4[2]), P(w), None) == 0
    bad = torch.tensor([-1, L, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    assert lib.pmenv_prio_update(P(tree), L, P(bad), P(w), 4, 0.6, 1e-6, None) == 0
    torch.cuda.synchronize()
    assert all((x == 0).all() for x in i4) and (w == 0).all() and torch.equal(tree, before)


# ---------------------------------------------------------------- exact sampling
def exact_cases():
    rng = np.random.default_rng(11)
    L = 64 * 70 + 5                                                          # not a multiple of 64; three levels
    p = rng.integers(0, 8, L)
    p[64 * 3:64 * 6] = 0                                                     # whole zero nodes
    p[64 * 10 - 7:64 * 10 + 9] = 0                                           # a zero run across a node border
    p[64 * 20] = 0                                                           # a node's first child
    p[-40:] = 0                                                              # zeros in the last positions, the ragged node whole
    yield "mixed", p
    p = np.zeros(L, dtype=np.int64)
    p[4000] = 50
    yield "single-leaf", p
    p = np.zeros(L, dtype=np.int64)
    p[L - 1] = 3
    p[0] = 2
    yield "first-and-last", p
    p = rng.integers(0, 5, 63)
    p[-3:] = 0
    yield "one-node", p
    p = rng.integers(1, 20, 262145) * (rng.random(262145) < 0.1)             # four levels, sparse
    p[-1] = 7
    yield "four-levels", p
    p = np.zeros(262145, dtype=np.int64)                                     # whole zero level-2 nodes before the only mass
    p[4096 * 40 + 17] = 1000
    p[262144] = 1
    yield "four-levels-sparse", p


@pytest.mark.parametrize("name,p", list(exact_cases()), ids=[n for n, _ in exact_cases()])
def test_gpu_prio_sampling_is_exact_for_integer_priorities(name, p):
    L, S = len(p), int(p.sum())
    assert 0 < S <= 2 ** 20
    tree = make_tree(p)
    _, lv = prio_ref.read_tree(tree, L)
    assert lv[-1].sum() == S                                                 # integers: every node is exact
    u = (np.arange(S) + 0.5) / S
    leaf, h0, env, w = sample(tree, L, u)
    assert np.array_equal(np.bincount(leaf, minlength=L), p)
    assert np.array_equal(leaf, np.repeat(np.arange(L), p))                  # and in target order
    assert np.array_equal(h0.astype(np.int64) * B + env, leaf) and (env >= 0).all() and (env < B).all()


# ---------------------------------------------------------------- bracket and weights
@functools.lru_cache(maxsize=None)
def random_tree(L):
    rng = np.random.default_rng(L + 1)
    vals = (rng.random(L) * np.exp(2 * rng.standard_normal(L))).astype(np.float32) + np.float32(1e-6)
    vals[rng.random(L) < 0.3] = 0.0                                          # about 30 % zeros
    vals[-70:] = 0.0
    vals[128:192] = 0.0
    tree = make_tree(vals)
    S = 2048
    u = np.concatenate([[0.0, np.nextafter(1.0, 0.0)], rng.random(S - 2)])
    return vals, tree, u


@pytest.mark.parametrize("L", [4485, 262145])
def test_gpu_prio_sample_brackets_its_target(L):
    vals, tree, u = random_tree(L)
    _, lv = prio_ref.read_tree(tree, L)
    prio_ref.check_levels(lv)
    total = lv[-1].sum()                                                     # read back from the device
    c = np.cumsum(vals.astype(np.float64))
    assert abs(total - c[-1]) <= 1e-12 * total
    Bn = 5
    assert L % Bn == 0
    leaf, h0, env, w = sample(tree, L, u, Bn=Bn)
    assert (leaf >= 0).all() and (leaf < L).all()
    assert (vals[leaf] > 0).all()                                            # hard: never a zero leaf
    t, tol = u * total, 1e-9 * total
    lo = np.where(leaf > 0, c[leaf - 1], 0.0)
    assert np.all(lo - tol <= t) and np.all(t <= c[leaf] + tol)
    assert leaf[0] == np.flatnonzero(vals)[0] and leaf[1] == np.flatnonzero(vals)[-1]   # u = 0 and u -> 1
    assert np.array_equal(h0.astype(np.int64) * Bn + env, leaf) and (env >= 0).all() and (env < Bn).all()


@pytest.mark.parametrize("L", [4485, 262145])
def test_gpu_prio_weights(L):
    vals, tree, u = random_tree(L)
    for beta in (0.4, 1.0):
        leaf, _, _, w = sample(tree, L, u, beta=beta)
        want = prio_ref.weights(vals[leaf], beta)
        assert w.dtype == np.float32 and np.all(np.abs(w - want) <= 1e-6 * want)
        assert w.max() == 1.0 and w[np.argmin(vals[leaf])] == 1.0 and (w > 0).all()
    leaf, _, _, w = sample(tree, L, u, beta=0.0)
    assert (w == 1.0).all()
    leaf1, _, _, w1 = sample(tree, L, u[:1], beta=0.7)                       # a batch of one: its own minimum
    assert w1[0] == 1.0


# ---------------------------------------------------------------- update
def open_tree(L):
    from pmenv.replay import prio_fill, prio_tree
    tree = prio_tree(L, DEV)
    prio_fill(tree, L, None, 0, L)
    return tree


def update(tree, L, idx, td, alpha=0.6, eps=1e-6):
    from pmenv.replay import prio_update
    prio_update(tree, L, dev(idx, torch.int32), dev(td, torch.float32), alpha, eps)


def test_gpu_prio_update_largest_duplicate_wins_in_either_order():
    L = 4485
    idx, td = [7, 7, 100, 7, 4484], [0.5, -2.0, 0.3, 1.0, 0.25]
    a, b = open_tree(L), open_tree(L)
    update(a, L, idx, td)
    update(b, L, idx[::-1], td[::-1])
    assert torch.equal(a, b)                                                 # bit-equal trees
    mx, lv = prio_ref.read_tree(a, L)
    p = prio_ref.priority(td, 0.6, 1e-6, 1.0)
    assert np.allclose(lv[0][[7, 100, 4484]], [p[1], p[2], p[4]], rtol=1e-6)
    assert np.allclose(mx, p[1], rtol=1e-6) and p[1] > 1.0
    prio_ref.check_levels(lv)
    update(a, L, [7, 7], [0.01, 0.02])                                       # the old value is no candidate
    _, lv = prio_ref.read_tree(a, L)
    assert np.allclose(lv[0][7], prio_ref.priority([0.02], 0.6, 1e-6, 1.0)[0], rtol=1e-6)
    prio_ref.check_levels(lv)


def test_gpu_prio_update_keeps_a_zero_leaf_zero():
    from pmenv.replay import prio_fill
    L = 4485
    tree = open_tree(L)
    prio_fill(tree, L, 64, None, 64)                                         # a whole node closes
    prio_fill(tree, L, 300, None, 1)
    before = tree.clone()
    update(tree, L, [70, 300, 70], [0.5, 0.25, 0.75])                        # new values below the maximum of 1
    assert torch.equal(tree, before)                                         # leaves, ancestors and maximum: the same bits
    update(tree, L, [70, 301], [0.5, 0.25])
    _, lv = prio_ref.read_tree(tree, L)
    assert lv[0][70] == 0.0 and lv[0][300] == 0.0 and lv[1][1] == 0.0 and 0.0 < lv[0][301] < 1.0
    prio_ref.check_levels(lv)


def test_gpu_prio_update_non_finite_td_gives_the_maximum_which_never_shrinks():
    L = 4485
    tree = open_tree(L)
    update(tree, L, [5], [3.0])
    mx, lv = prio_ref.read_tree(tree, L)
    assert mx == lv[0][5] and np.allclose(mx, prio_ref.priority([3.0], 0.6, 1e-6, 1.0)[0], rtol=1e-6) and mx > 1.0
    update(tree, L, [1, 2, 3, 4], [float("nan"), float("inf"), float("-inf"), 0.5])
    mx2, lv = prio_ref.read_tree(tree, L)
    assert mx2.view(np.int32) == mx.view(np.int32)                           # smaller and non-finite values: unchanged
    assert all(lv[0][i].view(np.int32) == mx.view(np.int32) for i in (1, 2, 3)) and lv[0][4] < 1.0
    prio_ref.check_levels(lv)
    update(tree, L, [9, 9], [7.0, 50.0])
    mx3, lv = prio_ref.read_tree(tree, L)
    assert mx3 > mx2 and mx3 == lv[0][9]
    update(tree, L, [9], [0.1])                                              # the maximum's own leaf drops: it stays
    mx4, lv = prio_ref.read_tree(tree, L)
    assert mx4 == mx3 and lv[0][9] < 1.0
    update(tree, L, [11], [3e38], alpha=2.0)                                 # overflowing f32: capped, finite
    mx5, lv = prio_ref.read_tree(tree, L)
    assert mx5 == np.finfo(np.float32).max and lv[0][11] == mx5
    update(tree, L, [12], [0.0], alpha=2.0, eps=0.0)                         # 0^2: raised to the smallest normal
    _, lv = prio_ref.read_tree(tree, L)
    assert lv[0][12] == np.finfo(np.float32).tiny


def test_gpu_prio_update_is_deterministic():
    L, S = 262145, 5000
    rng = np.random.default_rng(5)
    idx = np.concatenate([rng.integers(0, L, S - 500), rng.integers(0, 64, 500)])   # heavy duplicates in one node
    td = rng.standard_normal(S) * 4
    trees = []
    for _ in range(2):
        tree = open_tree(L)
        update(tree, L, idx, td)
        trees.append(tree)
    assert torch.equal(trees[0], trees[1])
    _, lv = prio_ref.read_tree(trees[0], L)
    prio_ref.check_levels(lv)


# ---------------------------------------------------------------- the replay's invariant
def filled_replay(N, W, F, check=None, **kw):
    """test_gpu_replay_seq.py's wrapped ring of three episodes, prioritized; check(rb) runs
    after every add."""
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay
    e2, e3 = 3 * W + 8, 2 * W + 3
    H = (W + 3) + e2 + e3
    e1 = H - 5
    T = 4 * W + 12
    rng = np.random.default_rng(N * 100 + W)
    bars = (100 * np.exp(0.01 * rng.standard_normal((T, N, F - 1)).cumsum(0))).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV), features=F, **kw)
    g = torch.Generator(device=DEV).manual_seed(N + W)
    env_off = torch.arange(B, dtype=torch.int32, device=DEV)
    for length, day0 in ((e1, -3 - (e1 - (W + 3))), (e2, W), (e3, T + 4 - e3 - (B - 1))):
        rb.new_episode()
        for k in range(length):
            rb.add(day0 + k + env_off, torch.rand(B, N, device=DEV, generator=g),
                   torch.randn(B, device=DEV, generator=g))
            if check is not None:
                check(rb)
    return rb


def open_leaves(rb):
    from pmenv.replay import valid_starts
    oldest = (rb.head - rb.count) % rb.H
    rows = sorted((oldest + int(st)) % rb.H for st in valid_starts(rb._row_ep, oldest, rb.count, rb.W, rb.H))
    return np.array([h * B + b for h in rows for b in range(B)], dtype=np.int64)


@pytest.mark.parametrize("N,W,F", [(4, 4, 5), (30, 50, 5)])
def test_gpu_replay_leaves_are_the_valid_starts_after_every_add(N, W, F):
    state = dict(prev=np.zeros(0, dtype=np.int64), counts=[], raised=False, grew=0, shrank=0)

    def check(rb):
        mx, lv = prio_ref.read_tree(rb.tree, rb.H * B)
        live = np.flatnonzero(lv[0])
        want = open_leaves(rb)
        assert np.array_equal(live, want), rb.count
        assert np.array_equal(np.flatnonzero(rb._row_open), np.unique(want // B))
        fresh = np.setdiff1d(live, state["prev"])
        assert (lv[0][fresh] == mx).all()                                    # a new start enters at the maximum
        state["grew"] += len(fresh) > 0
        state["shrank"] += len(np.setdiff1d(state["prev"], live)) > 0
        state["prev"] = live
        state["counts"].append(rb.count)
        if len(live) and not state["raised"]:                                # from the first start on, a larger maximum
            rb.update_priorities(torch.as_tensor(live[:1]), torch.tensor([5.0]))
            state["raised"] = True
        if len(state["counts"]) % 16 == 0 or rb.count in (W + 1, W + 2):
            prio_ref.check_levels(lv)

    rb = filled_replay(N, W, F, check=check, prioritized=True)
    H = rb.H
    assert state["counts"][W] == W + 1 and state["counts"][W + 1] == W + 2 and state["counts"][-1] == H
    assert state["counts"].count(H) > 5 and len(set(rb._row_ep)) == 3        # wrapped, three episodes left
    assert state["grew"] > H // 2 and state["shrank"] > 5
    mx, lv = prio_ref.read_tree(rb.tree, H * B)
    prio_ref.check_levels(lv)
    assert mx > 1.0 and (lv[0][open_leaves(rb)] >= 1.0).all()
    assert len(open_leaves(rb)) < (H - W - 1) * B                            # the episode boundaries cost starts


@functools.lru_cache(maxsize=None)
def replay_pair(N, W, F):
    return filled_replay(N, W, F, prioritized=True, alpha=1.0, eps=0.0), filled_replay(N, W, F)


@pytest.mark.parametrize("N,W,F", [(4, 4, 5), (30, 50, 5)])
def test_gpu_replay_sample_prioritized_is_the_gather_of_its_indices(N, W, F):
    rb, _ = replay_pair(N, W, F)
    S = 64
    u = (np.arange(S) + 0.5) / S
    h0, env, leaf, w = rb.prioritized_indices(S, u=u)
    assert h0.dtype == env.dtype == leaf.dtype == torch.int32 and w.dtype == torch.float32
    assert np.isin(leaf.cpu().numpy(), open_leaves(rb)).all() and len(torch.unique(leaf)) > S // 2
    assert torch.equal(h0 * B + env, leaf)
    got = rb.sample_prioritized(S, u=u)
    assert len(got) == 6 and torch.equal(got[4], leaf) and torch.equal(got[5], w)
    for x, y in zip(got[:4], rb.gather(h0, env)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    got = rb.sample_nstep_prioritized(S, 3, 0.9, u=u)
    assert len(got) == 8 and torch.equal(got[6], leaf) and torch.equal(got[7], w)
    for x, y in zip(got[:6], rb.gather_nstep(h0, env, 3, 0.9)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int(got[4].min()) >= 1 and int(got[4].max()) == 3
    if W == 4:
        assert int(got[4].min()) == 1                                        # nearly every leaf is drawn: short folds too
    # the stratified default: one sample per stratum of the total, from the generator as `indices` draws
    a = rb.prioritized_indices(S, generator=torch.Generator().manual_seed(1))
    b = rb.prioritized_indices(S, generator=torch.Generator().manual_seed(1))
    c = rb.prioritized_indices(S, generator=torch.Generator(device=DEV).manual_seed(1))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and np.isin(c[2].cpu().numpy(), open_leaves(rb)).all()
    assert (a[2][1:] >= a[2][:-1]).all() and len(torch.unique(a[2])) > S // 2


def test_gpu_replay_update_priorities_moves_the_sample_counts():
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay
    N, W, H = 4, 4, 20
    bars = np.random.default_rng(1).standard_normal((40, N, 4)).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV), prioritized=True, alpha=1.0, eps=0.0, beta=0.5,
                      beta_increment=0.3)
    with pytest.raises(ValueError):
        rb.prioritized_indices(4)
    for k in range(W + 1):
        rb.add(torch.full((B,), 5 + k), torch.rand(B, N), torch.randn(B))
    with pytest.raises(ValueError):
        rb.prioritized_indices(4)                                            # W + 1 rows: no start yet
    for k in range(W + 1, H):
        rb.add(torch.full((B,), 5 + k), torch.rand(B, N), torch.randn(B))
    live = open_leaves(rb)
    M = len(live)
    assert M == (H - W - 1) * B
    h0, env, leaf, w = rb.prioritized_indices(M, u=(np.arange(M) + 0.5) / M)
    assert np.array_equal(leaf.cpu().numpy(), live) and (w == 1.0).all()     # equal priorities: each leaf once
    x = int(live[7])
    rb.update_priorities(torch.tensor([x]), torch.tensor([-4.0]))
    S = M + 3
    h0, env, leaf, w = rb.prioritized_indices(S, u=(np.arange(S) + 0.5) / S)
    hist = np.bincount(leaf.cpu().numpy(), minlength=H * B)
    want = np.zeros(H * B, dtype=np.int64)
    want[live] = 1
    want[x] = 4
    assert np.array_equal(hist, want)
    assert rb.beta == 1.0                                                    # 0.5, 0.8, then capped
    wn = w.cpu().numpy()
    assert np.allclose(wn[leaf.cpu().numpy() == x], 4.0 ** -0.8, rtol=1e-6) and wn.max() == 1.0   # drawn at beta = 0.8
    # a leaf whose row has since been overwritten: the update changes nothing
    oldest = (rb.head - rb.count) % H
    stale = torch.tensor([oldest * B + 1, oldest * B + 2], dtype=torch.int32)
    rb.add(torch.full((B,), 5 + H), torch.rand(B, N), torch.randn(B))
    before = rb.tree.clone()
    rb.update_priorities(stale, torch.tensor([0.5, 3.0]))
    assert torch.equal(rb.tree, before)
    _, lv = prio_ref.read_tree(rb.tree, H * B)
    assert not lv[0][oldest * B:(oldest + 1) * B].any()
    with pytest.raises(ValueError):
        rb.update_priorities(stale, torch.tensor([1.0]))


def test_gpu_replay_prioritized_indices_raise_without_a_valid_start():
    from pmenv import MarketSeries
    from pmenv.replay import DeviceReplay
    N, W, H = 4, 4, 20
    bars = np.random.default_rng(1).standard_normal((40, N, 4)).astype(np.float32)
    rb = DeviceReplay(B, N, W, H, MarketSeries(bars, device=DEV), prioritized=True)
    for e in range(4):                                                       # episodes of W rows: none holds a window
        rb.new_episode()
        for k in range(W):
            rb.add(torch.full((B,), 5 + k), torch.rand(B, N), torch.randn(B))
    assert rb.count > W + 1 and len(open_leaves(rb)) == 0
    _, lv = prio_ref.read_tree(rb.tree, H * B)
    assert all(not x.view(np.uint8).any() for x in lv)
    with pytest.raises(ValueError):
        rb.prioritized_indices(4)
    with pytest.raises(ValueError):
        rb.indices(4)                                                        # as the uniform draw decides
    beta = rb.beta
    rb.new_episode()
    for k in range(W + 2):
        rb.add(torch.full((B,), 5 + k), torch.rand(B, N), torch.randn(B))
    h0, env, leaf, w = rb.prioritized_indices(4, u=[0.0, 0.3, 0.6, 0.9])
    assert rb.beta == beta and np.array_equal(leaf.cpu().numpy(), open_leaves(rb)[[0, 0, 1, 2]])   # one open row, B leaves


@pytest.mark.parametrize("N,W,F", [(4, 4, 5)])
def test_gpu_replay_unprioritized_is_unchanged(N, W, F):
    rb, plain = replay_pair(N, W, F)
    assert plain.tree is None and not plain.prioritized and rb.tree is not None
    for t in ("days", "actions", "rewards"):
        assert torch.equal(getattr(plain, t), getattr(rb, t))                # add stored the same rows
    assert plain.head == rb.head and plain.count == rb.count and np.array_equal(plain._row_ep, rb._row_ep)
    for make in (lambda: torch.Generator().manual_seed(9), lambda: torch.Generator(device=DEV).manual_seed(9)):
        a, b = plain.indices(200, generator=make()), rb.indices(200, generator=make())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for x, y in zip(plain.sample(50, generator=make()), rb.sample(50, generator=make())):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for call in (lambda: plain.prioritized_indices(4), lambda: plain.sample_prioritized(4),
                 lambda: plain.update_priorities(torch.zeros(1), torch.zeros(1))):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------- capture
def test_gpu_prio_sample_update_chain_is_graph_capturable():
    from pmenv.replay import prio_sample, prio_update
    L, S = 4485, 256
    vals, tree0, u_all = random_tree(L)
    u = dev(u_all[:S], torch.float64)
    td = dev(np.random.default_rng(3).standard_normal(S) * 2, torch.float32)
    tree = tree0.clone()
    eager = []
    for _ in range(2):
        out = prio_sample(tree, L, 5, u, 0.4)
        prio_update(tree, L, out[0], td, 0.6, 1e-6)
        eager.append([o.clone() for o in out] + [tree.clone()])
    assert not torch.equal(eager[0][4], eager[1][4]) and not torch.equal(eager[0][0], eager[1][0])
    tree.copy_(tree0)
    out = tuple(torch.zeros(S, dtype=torch.int32, device=DEV) for _ in range(3)) + (torch.zeros(S, device=DEV),)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        prio_sample(tree, L, 5, u, 0.4, out=out)
        prio_update(tree, L, out[0], td, 0.6, 1e-6)
    assert torch.equal(tree, tree0)                                          # captured, not run
    for want in eager:
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(out + (tree,), want):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ---------------------------------------------------------------- OffPolicy
def _loop(**kw):
    from pmenv import MarketSeries, TradingEnv
    from pmenv.off_policy import OffPolicy
    N, W, T = 7, 6, 200
    rng = np.random.default_rng(3)
    bars = (100 * np.exp(0.01 * rng.standard_normal((T, N, 4)).cumsum(0))).astype(np.float32)
    m = MarketSeries(bars, device=DEV)
    env = TradingEnv(num_envs=B, num_assets=N, window=W, device=DEV)
    return m, OffPolicy(env, m, capacity=40, batch_size=32, generator=torch.Generator().manual_seed(3), **kw)


@pytest.mark.parametrize("n_step", [1, 3])
def test_gpu_off_policy_prioritized_feeds_td_errors_back(n_step):
    seen = []

    def update_fn(*args):
        seen.append(args)
        return args[2].reshape(-1).abs()                                     # |r| as the TD error

    m, loop = _loop(update=update_fn, prioritized=True, alpha=0.7, beta=0.5, beta_increment=0.25, n_step=n_step)
    rb = loop.replay
    assert rb.prioritized and rb.alpha == 0.7 and rb.beta == 0.5
    g = torch.Generator().manual_seed(5)
    loop.collect(m.random_starts(B, 6, 16, generator=g), 16)
    loop.collect(m.random_starts(B, 6, 18, generator=g), 18)                 # a second episode in the ring
    H = rb.H
    live = open_leaves(rb)
    assert len(live) == ((16 - 6) + (18 - 6 - 1)) * B                        # the newest row completes no window yet
    state = loop.generator.get_state()
    h0, env, leaf, w = rb.prioritized_indices(32, loop.generator)            # the draw the update will make
    loop.generator.set_state(state)
    rb.beta = 0.5
    out = loop.update(1)
    assert len(seen) == 1 and len(seen[0]) == (5 if n_step == 1 else 6) and rb.beta == 0.75
    r, wgt = seen[0][2], seen[0][-1]
    assert r.shape == (32, 1, 1) and wgt.shape == (32,) and wgt.dtype == torch.float32
    assert torch.equal(wgt, w) and float(wgt.max()) == 1.0 and (wgt == 1.0).all()   # all leaves at 1 so far
    if n_step > 1:
        assert seen[0][4].shape == (32,)                                     # the discount goes before the weights
    assert torch.equal(out[0], r.reshape(-1).abs())
    leaf_h, td = leaf.cpu().numpy(), r.reshape(-1).abs().cpu().numpy()
    assert np.isin(leaf_h, live).all()
    new = prio_ref.priority(td, 0.7, 1e-6, 1.0)
    _, lv = prio_ref.read_tree(rb.tree, H * B)
    for i in np.unique(leaf_h):
        assert np.isclose(lv[0][i], new[leaf_h == i].max(), rtol=1e-6)
    rest = np.setdiff1d(live, leaf_h)
    assert (lv[0][rest] == 1.0).all() and np.array_equal(np.flatnonzero(lv[0]), live)
    prio_ref.check_levels(lv)


def test_gpu_off_policy_prioritized_with_sequences_raises():
    with pytest.raises(ValueError):
        _loop(prioritized=True, seq_len=8)
    _, loop = _loop()
    assert not loop.prioritized and loop.replay.tree is None
