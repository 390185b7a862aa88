"""Inputs, references and the raw-ABI caller of the replay gathers' edge tests
(test_replay_edges_host.py on the CPU, test_gpu_replay_gather_edges.py on the device).
Nothing here touches a device at import; torch is imported where a function needs it.

The rings are built in numpy as the ring stands after it wrapped: `oldest` mid-array,
count = H, several episodes, day indices off both ends of the series, one episode whose
days advance by two a row (the n-step gather's two-pass path and the sequence gather's
element-by-element path without m > W). The per-env ring moves every boundary by b rows in
column b and gives every column ids of its own.

Value references are the project's: oracle.replay_gather (s, a, r, s'), nstep_counts for m
(per column for a per-env ring), and the f64 Horner fold as test_gpu_replay_nstep.py
writes it."""
import ctypes
import functools
import math
import types

import numpy as np

B = 3                                    # envs of every ring
GUARD = 64                               # sentinel floats on either side of an output (256 B: keeps 16-B alignment)
SENTINEL = -7.5                          # no output holds it: bars > 0, actions in [0, 1), rewards drawn normal
ISENTINEL = -77                          # the same for steps / length
S_LABELS = ("1", "G", "G+1", "2G", "2G+1", "3G+1", "4G", "4G+1", "5G+1", "7G+2")


# 1. pipeline depth: (N, W, F) swept over S_LABELS, one-step and n in depth_n(W); the product's
# shape at 4G+1 alone
DEPTH_SHAPES = ((514, 2, 5), (300, 4, 5), (4, 4, 5))
DEPTH_ENV_SHAPES = ((514, 2, 5), (4, 4, 5))                 # .. and through pmenv_replay_gather_nstep_env at n = 2W + 3
PRODUCT = (30, 50, 5)
PRODUCT_N = ((5, "<8,2>"), (64, "<12,2>"))
SEQ_DEPTH = ((300, 4, 5), 11)                               # L = 11 at S = 5G + 1: Lc = 6, nc = 2, the last chunk short
# 2. pairs per thread: (N, W, n or L, S) and the instantiation
PPT_S = 70
PPT_ONE_STEP = (((32, 15), "<2,2>"), ((57, 8), "<4,2>"), ((64, 15), "<4,2>"), ((41, 24), "<8,2>"),
                ((128, 15), "<8,2>"), ((128, 16), "<8,2>"))
PPT_NSTEP = (((30, 50, 18), "<8,2>"), ((30, 50, 19), "<12,2>"), ((32, 48, 48), "<12,2>"), ((64, 47, 1), "<12,2>"),
             ((64, 47, 47), "<12,2>"))
PPT_SEQ = (((12, 40, 8, 200), "<4,16>"), ((40, 60, 16, 64), "<12,16>"), ((4, 4, 8, PPT_S), "<2,16>"),
           ((30, 50, 8, PPT_S), "<8,16>"))
# 3. store policy: (30, 50, 5), L = 64
POLICY_L, POLICY_S16, POLICY_S2 = 64, 139, 140
# 4. the fold
FOLD_N = (63, 64, 65, 127, 128, 129, 200)
FOLD_GAMMA = (0.9, 1.0)
FOLD_FORMS = (((4, 4, 5), "replay_nstep_f5p_kernel<2,2>"), ((3, 3, 3), "replay_nstep_lds_kernel"),
              ((257, 3, 5), "replay_nstep_kernel"))
FOLD_S = 16
GENERIC_S, ALIGN_S = 24, 28
# 5. generic-form boundaries: (kind, N, W, F, n) and the form
GENERIC = (("one_step", 64, 63, 4, 1, "lds"), ("nstep", 64, 63, 4, 1, "lds"),
           ("one_step", 64, 64, 4, 1, "elem"), ("nstep", 64, 64, 4, 1, "elem"),
           ("nstep", 64, 32, 4, 32, "lds"), ("nstep", 64, 33, 4, 33, "elem"),
           ("one_step", 256, 3, 3, 1, "lds"), ("nstep", 256, 3, 3, 3, "lds"),
           ("one_step", 257, 3, 3, 1, "elem"), ("nstep", 257, 3, 3, 3, "elem"), ("seq", 257, 3, 3, 4, "elem"),
           ("one_step", 5, 3, 3, 1, "lds"), ("nstep", 5, 3, 3, 3, "lds"), ("seq", 5, 3, 3, 4, "elem"))
# 6. alignment: `aligned` and the floats s / s_next / x and the series lie past a 16-B boundary
ALIGN_SHAPES = ((30, 12, 5), (30, 50, 5))
ALIGN_N = {"one_step": 1, "nstep": 5, "seq": 6}
ALIGN_OFFS = {2: (1, 0), 1: (0, 1), 0: (1, 1)}


def depth_n(W):
    return (1, W, 2 * W + 3)


def stem(kind):
    return {"one_step": "replay_gather", "nstep": "replay_nstep", "seq": "replay_seq"}[kind]


def parse(path):
    """pmenv_replay_path's string -> (kernel name, {field: text})"""
    name, *rest = path.split(" ")
    return name, dict(kv.split("=") for kv in rest)


def group_samples(path):
    """G, the samples a round of an f5p kernel's workgroups takes, from a path planned for a
    batch no grid is cut short by (S = 2^20)."""
    gx, gy = parse(path)[1]["grid"].split("x")
    return int(gx), int(gy)


def s_of(label, G):
    """A batch size of the pipeline-depth sweep from the samples G a round of workgroups takes."""
    return {"1": 1, "G": G, "G+1": G + 1, "2G": 2 * G, "2G+1": 2 * G + 1, "3G+1": 3 * G + 1, "4G": 4 * G,
            "4G+1": 4 * G + 1, "5G+1": 5 * G + 1, "7G+2": 7 * G + 2}[label]


def _frozen(a):
    a.flags.writeable = False
    return a


def _finish(c, chrono_days, chrono_ids, rng, oldest):
    """chronological rows -> the wrapped ring: row (oldest + i) % H holds chronological row i"""
    H, N = c.H, c.N
    c.oldest = oldest
    c.count = H
    c.span = H - c.W - 1
    roll = lambda a: _frozen(np.ascontiguousarray(np.roll(a, c.oldest, axis=0)))  # noqa: E731
    c.days = roll(chrono_days.astype(np.int32))
    c.ids = roll(chrono_ids.astype(np.int32))
    c.actions = _frozen(rng.random((H, B, N), dtype=np.float32))
    c.rewards = _frozen(rng.standard_normal((H, B)).astype(np.float32))          # mixed sign
    assert 0 < c.oldest < H
    return c


@functools.lru_cache(maxsize=None)
def edge_ring(N, W, F, per_env=False):
    """Four episodes, oldest first: W + 3 rows left of one the wrap cut (its windows begin
    before day 0), 3W + 8 rows, 2W + 6 rows whose days advance by two, 2W + 6 rows that end
    past the series. per_env: column b's boundaries lie b rows later and its ids are its
    own ([H, B]); else one id per row ([H])."""
    c = types.SimpleNamespace(N=N, W=W, F=F, per_env=per_env, B=B, T=4 * W + 12)
    rng = np.random.default_rng(1000 * N + 10 * W + F + (5 if per_env else 0))
    c.bars = _frozen((100 * np.exp(0.01 * rng.standard_normal((c.T, N, F - 1)).cumsum(0))).astype(np.float32))
    base = np.cumsum([0, W + 3, 3 * W + 8, 2 * W + 6, 2 * W + 6])
    c.H = H = int(base[-1])
    days = np.zeros((H, B), np.int64)
    ids = np.zeros((H, B), np.int64)
    c.bounds = []
    for b in range(B):
        cut = base.copy()
        cut[1:4] += b if per_env else 0
        c.bounds.append(tuple(int(x) for x in cut))
        for e in range(4):
            r = np.arange(cut[e + 1] - cut[e])
            day = (-3 + r, W + r, 5 + 2 * r, c.T + 4 - len(r) + r)[e] + b
            days[cut[e]:cut[e + 1], b] = day
            ids[cut[e]:cut[e + 1], b] = 3 + e + (10 * b if per_env else 0)
    # the array ends inside the windows of the second episode's last starts
    return _finish(c, days, ids if per_env else ids[:, 0], rng, 4 * W + 13)


@functools.lru_cache(maxsize=None)
def fold_ring(N, W, F):
    """One episode of W + 215 rows (215 starts: a start k rows before its last one folds
    k + 1 steps at the most) and a newer one of W + 10 rows; lockstep ids, days inside the series."""
    c = types.SimpleNamespace(N=N, W=W, F=F, per_env=False, B=B)
    rng = np.random.default_rng(77 * N + W + F)
    la, lb = W + 215, W + 10
    c.H = H = la + lb
    c.T = H + W + 8
    c.bars = _frozen((100 * np.exp(0.01 * rng.standard_normal((c.T, N, F - 1)).cumsum(0))).astype(np.float32))
    c.bounds = [(0, la, H)] * B
    days = (W + np.arange(H))[:, None] + np.arange(B)[None, :]
    ids = np.where(np.arange(H) < la, 8, 9)
    return _finish(c, days, ids, rng, H // 3 + 1)


def counts(c, st, env, n):
    """m of every start (offsets from the oldest row): nstep_counts, per column for a per-env ring."""
    from pmenv.replay import nstep_counts
    st, env = np.asarray(st, np.int64), np.asarray(env)
    if not c.per_env:
        return nstep_counts(c.ids, c.oldest, c.count, c.W, c.H, st, n)
    m = np.zeros(len(st), np.int32)
    for b in range(c.B):
        m[env == b] = nstep_counts(c.ids[:, b], c.oldest, c.count, c.W, c.H, st[env == b], n)
    return m


def candidates(c):
    """The starts an edge ring is sampled at, (st, env) with env = k % B: for each episode its
    first and last valid starts and the ones a few rows from them, so that folds and
    sequences are full, cut by an episode boundary and cut by the newest rows."""
    W, out = c.W, []
    picks = ((1, "first", 0), (1, "last", 0), (1, "last", -1), (1, "last", -W), (2, "first", 0), (2, "first", 1),
             (2, "last", -1), (2, "last", 0), (3, "last", 0), (3, "last", -1), (3, "last", -W), (3, "first", 0),
             (0, "first", 0), (0, "last", 0))
    for k, (e, end, d) in enumerate(picks):
        b = k % c.B
        cut = c.bounds[b]
        last = cut[e + 1] - W - 1 if e < 3 else c.span - 1      # the newest rows end the last episode's starts
        out.append(((cut[e] if end == "first" else last) + d, b))
    st, env = np.array(out).T
    return st.astype(np.int64), env.astype(np.int32)


@functools.lru_cache(maxsize=None)
def pattern(N, W, F, per_env, n):
    """The candidates in the order the pipeline sweeps take them for an n-step fold of n, with
    what the kernel decides for each: m, the uncapped run, whether s and s' share one image
    (joint) and why not (m > W, or days that skip). Order: joint, joint, two-pass, two-pass,
    joint, two-pass, .. — consecutive entries realise all four transitions."""
    c = edge_ring(N, W, F, per_env)
    st, env = candidates(c)
    m, run = counts(c, st, env, n), counts(c, st, env, 10 ** 6)
    h0 = (c.oldest + st) % c.H
    dA = c.days[(h0 + W - 1) % c.H, env].astype(np.int64) - (W - 1)
    dB = c.days[(h0 + m + W - 2) % c.H, env].astype(np.int64) + 1 - (W - 1)
    skips = dB - dA != m
    joint = ~skips & (m <= min(n, W))
    js, ts = list(np.flatnonzero(joint)), list(np.flatnonzero(~joint))
    order = js[:2] + ts[:2]
    js, ts = js[2:], ts[2:]
    while js or ts:
        order += js[:1] + ts[:1]
        js, ts = js[1:], ts[1:]
    o = np.array(order)
    p = types.SimpleNamespace(ring=c, n=n, K=len(o), st=st[o], env=env[o], h0=h0[o].astype(np.int32), m=m[o],
                              run=run[o], joint=joint[o], skips=skips[o], dA=dA[o], dB=dB[o])
    p.by_episode = (p.m == p.run) & (p.st + p.m < c.span)      # the fold ends at an episode boundary
    p.by_newest = (p.m == p.run) & (p.st + p.m == c.span)      # .. at the newest recorded rows
    return p


def slots(S, G, K, rot=0):
    """Pattern entry of every sample of a batch: workgroup g = j % G takes its samples
    j = g, g + G, .. in order and sees the pattern from entry g + rot on."""
    j = np.arange(S)
    return (j // G + j % G + rot) % K


def rotations(G, K):
    """One workgroup column alone (G = 1) repeats the batch with the pattern rotated, so that
    every entry passes every pipeline slot; wider grids have a workgroup per rotation."""
    return range(K) if G == 1 else (0,)


def fold_ref(c, h0, env, m, gamma):
    """(R, R with every step one fused multiply-add, discount, sum |g^k r_k|) in f64:
    acc = r_k + g * acc from the last term with g = float64(float32(gamma)), gamma^m as an
    m-fold product. The fused chain rounds the exact r_k + g * acc once a step (rationals)."""
    from fractions import Fraction
    g = np.float64(np.float32(gamma))
    R, Rf, disc, mag = (np.empty(len(h0)) for _ in range(4))
    for j in range(len(h0)):
        r = c.rewards[(int(h0[j]) + c.W - 1 + np.arange(m[j])) % c.H, env[j]].astype(np.float64)
        acc = fused = r[-1]
        for x in r[-2::-1]:
            acc = x + g * acc
            fused = np.float64(float(Fraction(float(x)) + Fraction(float(g)) * Fraction(float(fused))))
        d, a = np.float64(1.0), 0.0
        for k in range(m[j]):
            a += abs(d * r[k])
            d = d * g
        R[j], Rf[j], disc[j], mag[j] = acc, fused, d, a
    return R, Rf, disc, mag


def plain_sum(c, h0, env, m):
    return np.array([math.fsum(c.rewards[(int(h0[j]) + c.W - 1 + np.arange(m[j])) % c.H, env[j]].astype(np.float64))
                     for j in range(len(h0))])


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64).astype(np.float32))).astype(np.float64)


def fold_bound(ref, m, mag):
    """|R - f32(ref)| allowed: an f64 Horner chain of m steps, contracted or not (at most one
    rounding of 2^-53 relative a step, on partial sums within sum |g^k r_k|, taken twice over),
    plus one rounding to f32."""
    return ulp32(ref) + np.asarray(m, np.float64) * 2.0 ** -52 * mag


def expect(c, h0, env, m, gamma=0.9):
    """What the gathers return at the samples (h0, env) with folds of m steps: s, a, r of the
    one-step restatement (oracle.replay_gather), its s' (s_next1), s' at the last folded start
    (s_next), and the fold's f64 references."""
    from oracle import replay_gather
    h0, env, m = np.asarray(h0, np.int64), np.asarray(env, np.int32), np.asarray(m, np.int64)
    e = types.SimpleNamespace(h0=h0.astype(np.int32), env=env, m=m.astype(np.int32))
    e.s, e.a, e.r, e.s_next1 = replay_gather(c.bars, c.days, c.actions, c.rewards, h0, env, c.W)
    e.s_next = replay_gather(c.bars, c.days, c.actions, c.rewards, (h0 + m - 1) % c.H, env, c.W)[3]
    e.R, e.R_fused, e.disc, e.mag = fold_ref(c, h0, env, m, gamma)
    return e


@functools.lru_cache(maxsize=None)
def pattern_expect(N, W, F, per_env, n):
    """`expect` at the pattern's entries, in the pattern's order."""
    p = pattern(N, W, F, per_env, n)
    return expect(p.ring, p.h0, p.env, p.m)


@functools.lru_cache(maxsize=None)
def pattern_seq(N, W, F, per_env, L):
    """`seq_ref` at the pattern's entries: the pattern of an n-step fold of L is the sequence
    gather's too (length = m)."""
    p = pattern(N, W, F, per_env, L)
    return seq_ref(p.ring, p.h0, p.env, L)


@functools.lru_cache(maxsize=None)
def fold_expect(N, W, F, n, gamma):
    c = fold_ring(N, W, F)
    st, env = fold_starts(c)
    e = expect(c, (c.oldest + st) % c.H, env, counts(c, st, env, n), gamma)
    e.st, e.plain = st, plain_sum(c, e.h0, env, e.m)
    return e


def fold_starts(c):
    """Starts of the fold ring: the long episode's first two (every n up to 200 in full), the
    ones whose folds the boundary cuts to 129 .. 127 and 65 .. 63 and 1, and the newer episode's first and
    last."""
    la = c.bounds[0][1]
    last = la - c.W - 1                                   # the long episode's last valid start: m = 1
    st = np.array([0, 1, last - 128, last - 127, last - 126, last - 64, last - 63, last - 62, last, la, c.span - 1,
                   last - 199, 7, last - 1, la + 3, last - 65])
    return st.astype(np.int64), (np.arange(len(st)) % c.B).astype(np.int32)


def seq_ref(c, h0, env, L):
    """The sequence gather's outputs batch-major from the one-step restatement: (m, live [S, L],
    x [S, L, N, W, F], a [S, L, N], r [S, L]), dead elements +0.0."""
    from oracle import replay_gather
    S = len(h0)
    st = (np.asarray(h0, np.int64) - c.oldest) % c.H
    m = counts(c, st, env, L)
    live = np.arange(L)[None, :] < m[:, None]
    jj, tt = np.nonzero(live)
    s1, a1, r1, _ = replay_gather(c.bars, c.days, c.actions, c.rewards, (np.asarray(h0)[jj] + tt) % c.H,
                                  np.asarray(env)[jj], c.W)
    x = np.zeros((S, L, c.N, c.W, c.F), np.float32)
    a = np.zeros((S, L, c.N), np.float32)
    r = np.zeros((S, L), np.float32)
    x[jj, tt], a[jj, tt], r[jj, tt] = s1, a1, r1
    return m, live, x, a, r


# ---------------------------------------------------------------- the device side
def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _on_device(key, series_off):
    torch = _torch()
    c = key[0](*key[1:])
    dev = torch.device("cuda:0")
    d = types.SimpleNamespace()
    flat = torch.full((c.bars.size + 8,), float("inf"), device=dev)     # series_off floats past a 16-B boundary
    assert flat.data_ptr() % 16 == 0
    view = flat[series_off:series_off + c.bars.size]
    view.copy_(torch.as_tensor(np.array(c.bars).reshape(-1)))             # a copy: the ring's arrays are frozen
    d.bars = view
    assert d.bars.data_ptr() % 16 == 4 * series_off and d.bars.is_contiguous()
    for name in ("days", "actions", "rewards", "ids"):
        setattr(d, name, torch.as_tensor(np.array(getattr(c, name)), device=dev).contiguous())
    return d


def on_device(c, series_off=0):
    """The ring's arrays on cuda:0 (kept for the session); series_off = 1: the series 4 B past
    a 16-B boundary."""
    key = (fold_ring, c.N, c.W, c.F) if len(c.bounds[0]) == 3 else (edge_ring, c.N, c.W, c.F, c.per_env)
    return _on_device(key, series_off)


def guarded(n, off=0, dtype=None, fill=SENTINEL):
    """n output elements `off` elements past a 16-B boundary, between two runs of sentinels."""
    torch = _torch()
    raw = torch.full((n + 2 * GUARD + 4,), fill, device="cuda:0", dtype=dtype or torch.float32)
    assert raw.data_ptr() % 16 == 0
    view = raw[GUARD + off:GUARD + off + n]
    assert view.data_ptr() % 16 == 4 * off
    return raw, view


def assert_guards(raw, n, off=0, fill=SENTINEL, what="output"):
    lo, hi = raw[:GUARD + off], raw[GUARD + off + n:]
    assert hi.numel() >= GUARD
    assert bool((lo == fill).all()) and bool((hi == fill).all()), f"a store outside {what}"
    assert not bool((raw[GUARD + off:GUARD + off + n] == fill).any()), f"an element of {what} was not written"


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def call(kind, c, h0, env, n=1, gamma=0.9, L=1, time_major=False, out_off=0, series_off=0):
    """pmenv_replay_gather ("one_step"), _nstep / _nstep_env ("nstep") or _seq / _seq_env ("seq")
    through the raw ABI on ring c at the samples (h0, env) (numpy), the _env
    entry points for a per-env ring. Every output lies between 64 sentinels, s / s_next / x
    out_off floats past a 16-B boundary, the series series_off floats past one; the guards are
    asserted after the call. Returns the outputs as device views: s, s_next, a, r (, steps,
    discount) or x, a, r, length."""
    torch = _torch()
    from pmenv import _abi
    lib = _abi.load()
    d = on_device(c, series_off)
    h0, env = (torch.as_tensor(np.asarray(v, np.int32), device="cuda:0").contiguous() for v in (h0, env))
    S, N, W, F = h0.numel(), c.N, c.W, c.F
    per = N * W * F
    head = (_ptr(d.bars), c.T, N, F, W, _ptr(d.days), _ptr(d.actions), _ptr(d.rewards), c.H, c.B, _ptr(h0), _ptr(env),
            S)
    bufs = {}

    def out(name, count, off=0, integer=False):
        bufs[name] = (guarded(count, off, torch.int32, ISENTINEL) if integer else guarded(count, off)) + (count, off)
        return _ptr(bufs[name][1])

    if kind == "one_step":
        rc = lib.pmenv_replay_gather(*head, out("s", S * per, out_off), out("s_next", S * per, out_off),
                                     out("a", S * N), out("r", S), None)
        shapes = dict(s=(S, N, W, F), s_next=(S, N, W, F), a=(S, N), r=(S,))
    elif kind == "nstep":
        fn = lib.pmenv_replay_gather_nstep_env if c.per_env else lib.pmenv_replay_gather_nstep
        rc = fn(*head, _ptr(d.ids), c.oldest, c.count, n, gamma, out("s", S * per, out_off),
                out("s_next", S * per, out_off), out("a", S * N), out("r", S), out("steps", S, integer=True),
                out("discount", S), None)
        shapes = dict(s=(S, N, W, F), s_next=(S, N, W, F), a=(S, N), r=(S,), steps=(S,), discount=(S,))
    else:
        fn = lib.pmenv_replay_gather_seq_env if c.per_env else lib.pmenv_replay_gather_seq
        lead = (L, S) if time_major else (S, L)
        rc = fn(*head, _ptr(d.ids), c.oldest, c.count, L, 1 if time_major else 0, out("x", S * L * per, out_off),
                out("a", S * L * N), out("r", S * L), out("length", S, integer=True), None)
        shapes = dict(x=lead + (N, W, F), a=lead + (N,), r=lead, length=(S,))
    assert rc == 0, f"{kind}: rc = {rc}"
    torch.cuda.synchronize()
    res = types.SimpleNamespace()
    for name, (raw, view, count, off) in bufs.items():
        integer = view.dtype == torch.int32
        assert_guards(raw, count, off, ISENTINEL if integer else SENTINEL, f"{kind} {name}")
        setattr(res, name, view.view(*shapes[name]))
    return res


def canon_d(x):
    """device float32 -> int32 bits with one NaN for all"""
    torch = _torch()
    x = x.contiguous()
    return torch.where(torch.isnan(x), torch.full_like(x, float("nan")), x).view(torch.int32)


def same_bits(got, want):
    """bit equality on the device, any NaN for any NaN; want: a device tensor or numpy"""
    torch = _torch()
    if not torch.is_tensor(want):
        want = torch.as_tensor(np.ascontiguousarray(want), device=got.device)
    return got.shape == want.shape and torch.equal(canon_d(got), canon_d(want))
