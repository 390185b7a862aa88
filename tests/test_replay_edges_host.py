"""The conditions test_gpu_replay_gather_edges.py relies on, on the CPU: what the rings and the
start lists of replay_edge_inputs.py contain (the transitions between consecutive samples of
a workgroup, the folds cut by an episode boundary and by the newest rows at every pipeline
slot, the m values of the fold cases, windows off both ends of the series), and the full
pmenv_replay_path string of every shape of the GPU cases at cus = 256 — the kernel
instantiation, the asset group, the staged days, the grid and the LDS bytes, written out by
hand from csrc/replay_plan.h's rules."""
import numpy as np
import pytest

import replay_edge_inputs as E
from pmenv.replay import gather_path, valid_pairs
from replay_env_inputs import record

CUS = 256

# (kind, N, W, F, n or L, S, aligned) -> the plan at 256 compute units
PATHS = {
    # 1. pipeline depth, at S = 4G + 1 (the other batch sizes change the grid's x alone)
    ("one_step", 514, 2, 5, 1, 5, 3): "replay_gather_f5p_kernel<2,2> R=2 D=3 grid=1x257 lds=120",
    ("nstep", 514, 2, 5, 1, 5, 3): "replay_nstep_f5p_kernel<2,2> R=2 D=3 grid=1x257 lds=120",
    ("nstep", 514, 2, 5, 2, 5, 3): "replay_nstep_f5p_kernel<2,2> R=2 D=4 grid=1x257 lds=160",
    ("nstep", 514, 2, 5, 7, 5, 3): "replay_nstep_f5p_kernel<2,2> R=2 D=4 grid=1x257 lds=160",
    ("one_step", 300, 4, 5, 1, 513, 3): "replay_gather_f5p_kernel<4,2> R=150 D=5 grid=128x2 lds=15000",
    ("nstep", 300, 4, 5, 1, 513, 3): "replay_nstep_f5p_kernel<4,2> R=150 D=5 grid=128x2 lds=15000",
    ("nstep", 300, 4, 5, 4, 513, 3): "replay_nstep_f5p_kernel<8,2> R=150 D=8 grid=128x2 lds=24000",
    ("nstep", 300, 4, 5, 11, 513, 3): "replay_nstep_f5p_kernel<8,2> R=150 D=8 grid=128x2 lds=24000",
    ("one_step", 4, 4, 5, 1, 1025, 3): "replay_gather_f5p_kernel<2,2> R=4 D=5 grid=256x1 lds=400",
    ("nstep", 4, 4, 5, 1, 1025, 3): "replay_nstep_f5p_kernel<2,2> R=4 D=5 grid=256x1 lds=400",
    ("nstep", 4, 4, 5, 4, 1025, 3): "replay_nstep_f5p_kernel<2,2> R=4 D=8 grid=256x1 lds=640",
    ("nstep", 4, 4, 5, 11, 1025, 3): "replay_nstep_f5p_kernel<2,2> R=4 D=8 grid=256x1 lds=640",
    ("nstep", 30, 50, 5, 5, 1025, 3): "replay_nstep_f5p_kernel<8,2> R=30 D=55 grid=256x1 lds=33000",
    ("nstep", 30, 50, 5, 64, 1025, 3): "replay_nstep_f5p_kernel<12,2> R=30 D=100 grid=256x1 lds=60000",
    ("seq", 300, 4, 5, 11, 641, 3): "replay_seq_f5p_kernel<8,16> R=150 D=10 Lc=6 nc=2 grid=256x1 lds=30016",
    # 2. pairs per thread
    ("one_step", 32, 15, 5, 1, 70, 3): "replay_gather_f5p_kernel<2,2> R=32 D=16 grid=70x1 lds=10240",
    ("one_step", 57, 8, 5, 1, 70, 3): "replay_gather_f5p_kernel<4,2> R=57 D=9 grid=70x1 lds=10260",
    ("one_step", 64, 15, 5, 1, 70, 3): "replay_gather_f5p_kernel<4,2> R=64 D=16 grid=70x1 lds=20480",
    ("one_step", 41, 24, 5, 1, 70, 3): "replay_gather_f5p_kernel<8,2> R=41 D=25 grid=70x1 lds=20500",
    ("one_step", 128, 15, 5, 1, 70, 3): "replay_gather_f5p_kernel<8,2> R=128 D=16 grid=70x1 lds=40960",
    ("one_step", 128, 16, 5, 1, 70, 3): "replay_gather_f5p_kernel<8,2> R=64 D=17 grid=70x2 lds=21760",
    ("nstep", 30, 50, 5, 18, 70, 3): "replay_nstep_f5p_kernel<8,2> R=30 D=68 grid=70x1 lds=40800",
    ("nstep", 30, 50, 5, 19, 70, 3): "replay_nstep_f5p_kernel<12,2> R=30 D=69 grid=70x1 lds=41400",
    ("nstep", 32, 48, 5, 48, 70, 3): "replay_nstep_f5p_kernel<12,2> R=32 D=96 grid=70x1 lds=61440",
    ("nstep", 64, 47, 5, 1, 70, 3): "replay_nstep_f5p_kernel<12,2> R=64 D=48 grid=70x1 lds=61440",
    ("nstep", 64, 47, 5, 47, 70, 3): "replay_nstep_f5p_kernel<12,2> R=32 D=94 grid=70x2 lds=60160",
    ("seq", 12, 40, 5, 8, 200, 3): "replay_seq_f5p_kernel<4,16> R=12 D=44 Lc=4 nc=2 grid=256x1 lds=10576",
    ("seq", 40, 60, 5, 16, 64, 3): "replay_seq_f5p_kernel<12,16> R=40 D=64 Lc=4 nc=4 grid=256x1 lds=51216",
    ("seq", 4, 4, 5, 8, 70, 3): "replay_seq_f5p_kernel<2,16> R=4 D=6 Lc=2 nc=4 grid=256x1 lds=496",
    ("seq", 30, 50, 5, 8, 70, 3): "replay_seq_f5p_kernel<8,16> R=30 D=52 Lc=2 nc=4 grid=256x1 lds=31216",
    # 3. the sequence gather's store policy, and the one-step gather its elements are held to
    ("seq", 30, 50, 5, 64, 139, 3): "replay_seq_f5p_kernel<8,16> R=30 D=58 Lc=8 nc=8 grid=256x1 lds=34816",
    ("seq", 30, 50, 5, 64, 140, 3): "replay_seq_f5p_kernel<8,2> R=30 D=58 Lc=8 nc=8 grid=256x1 lds=34816",
    ("one_step", 30, 50, 5, 1, 8960, 3): "replay_gather_f5p_kernel<8,2> R=30 D=51 grid=256x1 lds=30600",
    # 5. generic-form boundaries
    ("one_step", 64, 63, 4, 1, 24, 3): "replay_gather_lds_kernel R=0 D=64 grid=24x1 lds=65536",
    ("nstep", 64, 63, 4, 1, 24, 3): "replay_nstep_lds_kernel R=0 D=64 grid=24x1 lds=65536",
    ("one_step", 64, 64, 4, 1, 24, 3): "replay_gather_kernel R=0 grid=1536x1 lds=0",
    ("nstep", 64, 64, 4, 1, 24, 3): "replay_nstep_kernel R=0 grid=1536x1 lds=0",
    ("nstep", 64, 32, 4, 32, 24, 3): "replay_nstep_lds_kernel R=0 D=64 grid=24x1 lds=65536",
    ("nstep", 64, 33, 4, 33, 24, 3): "replay_nstep_kernel R=0 grid=792x1 lds=0",
    ("one_step", 256, 3, 3, 1, 24, 3): "replay_gather_lds_kernel R=0 D=4 grid=24x1 lds=12288",
    ("nstep", 256, 3, 3, 3, 24, 3): "replay_nstep_lds_kernel R=0 D=6 grid=24x1 lds=18432",
    ("one_step", 257, 3, 3, 1, 24, 3): "replay_gather_kernel R=0 grid=217x1 lds=0",
    ("nstep", 257, 3, 3, 3, 24, 3): "replay_nstep_kernel R=0 grid=217x1 lds=0",
    ("seq", 257, 3, 3, 4, 24, 3): "replay_seq_kernel R=0 grid=868x1 lds=0",
    ("one_step", 5, 3, 3, 1, 24, 3): "replay_gather_lds_kernel R=0 D=4 grid=24x1 lds=240",
    ("nstep", 5, 3, 3, 3, 24, 3): "replay_nstep_lds_kernel R=0 D=6 grid=24x1 lds=360",
    ("seq", 5, 3, 3, 4, 24, 3): "replay_seq_kernel R=0 grid=17x1 lds=0",
    # 6. alignment: both 16-B aligned, s / s_next / x 4 B off, the series 4 B off, both
    ("one_step", 30, 12, 5, 1, 28, 3): "replay_gather_f5p_kernel<2,2> R=30 D=13 grid=28x1 lds=7800",
    ("one_step", 30, 12, 5, 1, 28, 2): "replay_gather_kernel R=0 grid=197x1 lds=0",
    ("one_step", 30, 12, 5, 1, 28, 1): "replay_gather_lds_kernel R=0 D=13 grid=28x1 lds=7800",
    ("one_step", 30, 12, 5, 1, 28, 0): "replay_gather_kernel R=0 grid=197x1 lds=0",
    ("nstep", 30, 12, 5, 5, 28, 3): "replay_nstep_f5p_kernel<2,2> R=30 D=17 grid=28x1 lds=10200",
    ("nstep", 30, 12, 5, 5, 28, 2): "replay_nstep_kernel R=0 grid=197x1 lds=0",
    ("nstep", 30, 12, 5, 5, 28, 1): "replay_nstep_lds_kernel R=0 D=17 grid=28x1 lds=10200",
    ("nstep", 30, 12, 5, 5, 28, 0): "replay_nstep_kernel R=0 grid=197x1 lds=0",
    ("seq", 30, 12, 5, 6, 28, 3): "replay_seq_f5p_kernel<2,16> R=30 D=13 Lc=1 nc=6 grid=168x1 lds=7816",
    ("seq", 30, 12, 5, 6, 28, 2): "replay_seq_kernel R=0 grid=1182x1 lds=0",
    ("seq", 30, 12, 5, 6, 28, 1): "replay_seq_kernel R=0 grid=1182x1 lds=0",
    ("seq", 30, 12, 5, 6, 28, 0): "replay_seq_kernel R=0 grid=1182x1 lds=0",
    ("one_step", 30, 50, 5, 1, 28, 3): "replay_gather_f5p_kernel<8,2> R=30 D=51 grid=28x1 lds=30600",
    ("one_step", 30, 50, 5, 1, 28, 2): "replay_gather_kernel R=0 grid=821x1 lds=0",
    ("one_step", 30, 50, 5, 1, 28, 1): "replay_gather_lds_kernel R=0 D=51 grid=28x1 lds=30600",
    ("one_step", 30, 50, 5, 1, 28, 0): "replay_gather_kernel R=0 grid=821x1 lds=0",
    ("nstep", 30, 50, 5, 5, 28, 3): "replay_nstep_f5p_kernel<8,2> R=30 D=55 grid=28x1 lds=33000",
    ("nstep", 30, 50, 5, 5, 28, 2): "replay_nstep_kernel R=0 grid=821x1 lds=0",
    ("nstep", 30, 50, 5, 5, 28, 1): "replay_nstep_lds_kernel R=0 D=55 grid=28x1 lds=33000",
    ("nstep", 30, 50, 5, 5, 28, 0): "replay_nstep_kernel R=0 grid=821x1 lds=0",
    ("seq", 30, 50, 5, 6, 28, 3): "replay_seq_f5p_kernel<8,16> R=30 D=51 Lc=1 nc=6 grid=168x1 lds=30616",
    ("seq", 30, 50, 5, 6, 28, 2): "replay_seq_kernel R=0 grid=4922x1 lds=0",
    ("seq", 30, 50, 5, 6, 28, 1): "replay_seq_kernel R=0 grid=4922x1 lds=0",
    ("seq", 30, 50, 5, 6, 28, 0): "replay_seq_kernel R=0 grid=4922x1 lds=0",
}
# 4. the fold: n changes nothing in these plans (D = W + min(n, W) = 2W from n = W on)
FOLD_PATHS = {(4, 4, 5): "replay_nstep_f5p_kernel<2,2> R=4 D=8 grid=16x1 lds=640",
              (3, 3, 3): "replay_nstep_lds_kernel R=0 D=6 grid=16x1 lds=216",
              (257, 3, 5): "replay_nstep_kernel R=0 grid=241x1 lds=0"}
# the samples a round of workgroups takes, and the asset groups per sample, at 256 compute units
GROUPS = {(514, 2, 5): (1, 257), (300, 4, 5): (128, 2), (4, 4, 5): (256, 1), (30, 50, 5): (256, 1)}


def path(kind, N, W, F, n, S, aligned=3):
    return gather_path(kind, N, W, F, n=n, S=S, aligned=aligned, cus=CUS)


# ---------------------------------------------------------------- the plans
def test_every_shape_of_the_gpu_cases_has_its_plan_pinned():
    for key, want in PATHS.items():
        assert path(*key) == want, key
    for (N, W, F), want in FOLD_PATHS.items():
        for n in E.FOLD_N:
            assert path("nstep", N, W, F, n, E.FOLD_S) == want, (N, W, F, n)
    # every table of the GPU cases is pinned above, under the name the table gives it
    for (N, W), inst in E.PPT_ONE_STEP:
        assert PATHS["one_step", N, W, 5, 1, E.PPT_S, 3].startswith(f"replay_gather_f5p_kernel{inst} ")
    for (N, W, n), inst in E.PPT_NSTEP:
        assert PATHS["nstep", N, W, 5, n, E.PPT_S, 3].startswith(f"replay_nstep_f5p_kernel{inst} ")
    for (N, W, L, S), inst in E.PPT_SEQ:
        assert PATHS["seq", N, W, 5, L, S, 3].startswith(f"replay_seq_f5p_kernel{inst} ")
    for n, inst in E.PRODUCT_N:
        assert PATHS[("nstep",) + E.PRODUCT + (n, 1025, 3)].startswith(f"replay_nstep_f5p_kernel{inst} ")
    for (shape, name) in E.FOLD_FORMS:
        assert FOLD_PATHS[shape].startswith(name + " ")
    for kind, N, W, F, n, form in E.GENERIC:
        name = E.stem(kind) + ("_lds_kernel" if form == "lds" else "_kernel")
        assert PATHS[kind, N, W, F, n, E.GENERIC_S, 3].startswith(name + " ")
    for (N, W, F) in E.ALIGN_SHAPES:
        for kind, n in E.ALIGN_N.items():
            for aligned in (3, 2, 1, 0):
                got = E.parse(PATHS[kind, N, W, F, n, E.ALIGN_S, aligned])[0]
                lds = "replay_seq_kernel" if kind == "seq" else E.stem(kind) + "_lds_kernel"
                want = {3: E.stem(kind) + "_f5p_kernel<", 2: E.stem(kind) + "_kernel", 1: lds,
                        0: E.stem(kind) + "_kernel"}[aligned]
                assert got.startswith(want) and (aligned == 3 or got == want), (kind, N, W, aligned, got)


def test_the_pairs_per_thread_shapes_sit_on_the_ladder_s_rungs():
    """A full shape has R * D an exact multiple of 256, a +1 shape one pair more."""
    pairs = lambda p: int(E.parse(p)[1]["R"]) * int(E.parse(p)[1]["D"])  # noqa: E731
    one = [pairs(PATHS["one_step", N, W, 5, 1, E.PPT_S, 3]) for (N, W), _ in E.PPT_ONE_STEP]
    assert one[:5] == [512, 513, 1024, 1025, 2048] and one[5] == 64 * 17
    nst = [pairs(PATHS["nstep", N, W, 5, n, E.PPT_S, 3]) for (N, W, n), _ in E.PPT_NSTEP]
    assert nst == [2040, 2070, 3072, 3072, 32 * 94]
    assert 128 * 17 > 2048 and 64 * 94 > 3072                                # why the two shapes split into two groups


def test_the_depth_sweeps_reach_every_pipeline_depth_at_their_group_sizes():
    for shape in E.DEPTH_SHAPES + (E.PRODUCT,):
        N, W, F = shape
        G, gy = GROUPS[shape]
        assert gy == max(N // int(E.parse(path("one_step", N, W, F, 1, 1))[1]["R"]), 1) and G == max(CUS // gy, 1)
        for kind, n in [("one_step", 1)] + [("nstep", n) for n in E.depth_n(W)]:
            assert E.group_samples(path(kind, N, W, F, n, 2 ** 20)) == (G, gy)
            if shape == E.PRODUCT:
                continue
            pinned = PATHS[kind, N, W, F, n, 4 * G + 1, 3]
            for label in E.S_LABELS:
                S = E.s_of(label, G)
                want = pinned.replace(f"grid={G}x", f"grid={min(S, G)}x")
                assert path(kind, N, W, F, n, S) == want, (shape, n, label)
    sizes = [E.s_of(label, 128) for label in E.S_LABELS]
    assert sizes == [1, 128, 129, 256, 257, 385, 512, 513, 641, 898]
    # samples of the deepest workgroup: 1 .. 4 (the chain's prologue alone), 5, 6 and 8 (the rotation)
    assert [-(-s // 128) for s in sizes] == [1, 1, 2, 2, 3, 4, 4, 5, 6, 8]
    assert GROUPS[300, 4, 5][1] == 2                       # more than one asset group with more than one sample each


# ---------------------------------------------------------------- the rings
RINGS = sorted({(s, False) for s in E.DEPTH_SHAPES + (E.PRODUCT,) + E.ALIGN_SHAPES} |
               {(s, True) for s in E.DEPTH_ENV_SHAPES + (E.SEQ_DEPTH[0],)} |
               {((N, W, 5), False) for (N, W), _ in E.PPT_ONE_STEP} |
               {((N, W, 5), False) for (N, W, _), _ in E.PPT_NSTEP} |
               {((N, W, 5), False) for (N, W, _, _), _ in E.PPT_SEQ} |
               {((N, W, F), False) for _, N, W, F, _, _ in E.GENERIC})
RING_IDS = [f"{'x'.join(map(str, s))}{'-env' if e else ''}" for s, e in RINGS]


@pytest.mark.parametrize("shape,per_env", RINGS, ids=RING_IDS)
def test_edge_ring_is_wrapped_holds_four_episodes_and_leaves_the_series_at_both_ends(shape, per_env):
    N, W, F = shape
    c = E.edge_ring(N, W, F, per_env)
    H = c.H
    assert c.count == H == 8 * W + 23 and 0 < c.oldest < H - 1 and c.span == H - W - 1
    assert c.days.shape == (H, E.B) and c.actions.shape == (H, E.B, N) and c.rewards.shape == (H, E.B)
    assert c.ids.shape == ((H, E.B) if per_env else (H,)) and c.ids.dtype == np.int32
    chrono = np.roll(c.ids, -c.oldest, axis=0).reshape(H, -1)
    assert (np.diff(chrono, axis=0) >= 0).all() and ((np.diff(chrono, axis=0) > 0).sum(0) == 3).all()
    assert chrono[0, 0] > 0                                                  # the ring came round: no id 0 is left
    if per_env:                                                              # every column ends its episodes elsewhere
        ends = [tuple(np.flatnonzero(np.diff(chrono[:, b]))) for b in range(E.B)]
        assert len(set(ends)) == E.B and len({chrono[0, b] for b in range(E.B)}) == E.B
    assert (c.rewards > 0).any() and (c.rewards < 0).any()
    st, env = E.candidates(c)
    assert len(set(zip(st.tolist(), env.tolist()))) == len(st) == 14 and set(env.tolist()) == set(range(E.B))
    h0 = (c.oldest + st) % H
    assert (h0 + W >= H).any() and (h0 + W < H).any()                        # windows across the array's end, and not
    first = c.days[(h0 + W - 1) % H, env] - (W - 1)
    assert (first < 0).any() and (first + W >= c.T).any() and ((first >= 0) & (first + W < c.T)).any()
    E.counts(c, st, env, 1)                                                  # raises on a start that is not valid
    # the third episode's days advance by two a row, the others' by one
    for b in range(E.B):
        cut = c.bounds[b]
        d = np.roll(c.days[:, b], -c.oldest)
        for e in range(4):
            assert (np.diff(d[cut[e]:cut[e + 1]]) == (2 if e == 2 else 1)).all()


@pytest.mark.parametrize("shape", E.DEPTH_ENV_SHAPES + (E.SEQ_DEPTH[0],), ids=lambda s: "x".join(map(str, s)))
def test_per_env_counts_agree_with_the_recorded_ring_model(shape):
    """m of the per-env ring against replay_env_inputs.record and valid_pairs: the ring recorded
    row by row from the done flags its boundaries stand for, unwrapped."""
    N, W, F = shape
    c = E.edge_ring(N, W, F, True)
    H = c.H
    done = np.zeros((H, E.B), bool)
    for b in range(E.B):
        done[np.array(c.bounds[b][1:4]) - 1, b] = True
    ep, head, count = record(done, H)
    assert head == 0 and count == H
    ok = np.zeros((c.span + 1, E.B), bool)
    pairs = valid_pairs(ep, 0, H, W + 1, H)
    ok[pairs[:, 0], pairs[:, 1]] = True
    st, env = E.candidates(c)
    for n in E.depth_n(W) + (E.SEQ_DEPTH[1],):
        m = E.counts(c, st, env, n)
        for s, b, mj in zip(st, env, m):
            run = 0
            while run < n and ok[s + run, b]:
                run += 1
            assert run == mj >= 1, (s, b, n)


# ---------------------------------------------------------------- the start lists
def _transitions(joint):
    return {(bool(a), bool(b)) for a, b in zip(joint[:-1], joint[1:])}


PATTERNS = [(s, False, n) for s in E.DEPTH_SHAPES for n in E.depth_n(s[1])] + \
           [(E.PRODUCT, False, n) for n, _ in E.PRODUCT_N] + \
           [(s, True, 2 * s[1] + 3) for s in E.DEPTH_ENV_SHAPES] + \
           [(E.SEQ_DEPTH[0], e, E.SEQ_DEPTH[1]) for e in (False, True)]


@pytest.mark.parametrize("shape,per_env,n", PATTERNS,
                         ids=[f"{'x'.join(map(str, s))}{'-env' if e else ''}-n{n}" for s, e, n in PATTERNS])
def test_start_list_realises_every_transition_and_every_way_a_fold_ends(shape, per_env, n):
    N, W, F = shape
    p = E.pattern(N, W, F, per_env, n)
    assert p.K == 14 and (p.m >= 1).all() and (p.m <= n).all()
    assert (p.m == n).any() and p.by_episode.any() and p.by_newest.any()     # a full fold, and both ways to end early
    if n == 1:
        assert p.joint.all()
        return
    assert ((p.m < n) & p.by_episode).any() and ((p.m < n) & p.by_newest).any()
    # joint -> joint, joint -> two-pass, two-pass -> two-pass, two-pass -> joint within five samples
    assert list(p.joint[:5]) == [True, True, False, False, True]
    assert _transitions(p.joint[:5]) == {(True, True), (True, False), (False, False), (False, True)}
    assert (p.skips & ~p.joint & (p.m <= W)).any()                           # two passes by days that skip alone
    assert (p.joint & (p.m > 1)).any()                                       # one image for a fold of several steps
    if n > W:
        assert (~p.skips & (p.m > W)).any()                                  # two passes by m > W, the days in step
    assert (p.dB - p.dA == p.m)[~p.skips].all()


@pytest.mark.parametrize("shape", E.DEPTH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_pipeline_slot_sees_both_cuts_and_every_transition(shape):
    """Sample j is the (j // G)-th of workgroup j % G: the first four come from the chain's
    prologue, every later one through the rotated slots. At the two deepest sweeps every slot
    holds a fold cut by an episode boundary and one cut by the newest rows, and the samples
    that follow one another in a workgroup realise all four transitions into every slot."""
    N, W, F = shape
    G, _ = GROUPS[shape]
    sweeps = [(False, n) for n in E.depth_n(W)[1:]] + [(True, 2 * W + 3)] * (shape in E.DEPTH_ENV_SHAPES)
    for per_env, n in sweeps:
        p = E.pattern(N, W, F, per_env, n)
        for label in ("5G+1", "7G+2"):
            S = E.s_of(label, G)
            depth = -(-S // G)
            seen = {d: set() for d in range(depth)}
            trans = {d: set() for d in range(1, depth)}
            for rot in E.rotations(G, p.K):
                k = E.slots(S, G, p.K, rot)
                for j in range(S):
                    seen[j // G].add(int(k[j]))
                    if j >= G:
                        trans[j // G].add((bool(p.joint[k[j - G]]), bool(p.joint[k[j]])))
            full = depth - 1 if S % G else depth                             # slots every workgroup reaches
            for d in range(min(full, 5) if G > 1 else depth):
                ks = np.array(sorted(seen[d]))
                assert p.by_episode[ks].any() and p.by_newest[ks].any(), (n, label, d)
                assert d == 0 or len(trans[d]) == 4, (n, label, d)
            assert depth >= 6


def test_rotations_and_slots():
    assert list(E.rotations(1, 14)) == list(range(14)) and list(E.rotations(128, 14)) == [0]
    k = E.slots(9, 1, 14, 3)
    assert list(k) == [3, 4, 5, 6, 7, 8, 9, 10, 11]                          # one workgroup: the pattern in order
    k = E.slots(7, 3, 14)
    assert list(k) == [0, 1, 2, 1, 2, 3, 2]                                  # workgroup g starts at entry g


def test_sequence_depth_case_has_a_short_last_chunk_and_every_kind_of_sequence():
    (N, W, F), L = E.SEQ_DEPTH
    f = E.parse(PATHS["seq", N, W, F, L, 641, 3])[1]
    Lc, nc = int(f["Lc"]), int(f["nc"])
    assert (Lc, nc) == (6, 2) and (nc - 1) * Lc < L < nc * Lc                # the last chunk holds 5 elements
    for per_env in (False, True):
        p = E.pattern(N, W, F, per_env, L)
        assert (p.m == L).any() and (p.m <= Lc).any() and ((p.m > Lc) & (p.m < L)).any()   # cut in either chunk
        # chunks staged element by element, and at once
        assert (p.skips & (p.m > 1)).any() and (~p.skips & (p.m > 1)).any()
        m, live, x, a, r = E.pattern_seq(N, W, F, per_env, L)
        assert np.array_equal(m, p.m) and np.isnan(x[live]).any() and not x[~live].view(np.int32).any()


def test_store_policy_sizes_straddle_256_mib():
    N, W, F = E.PRODUCT
    size = lambda S: S * E.POLICY_L * N * W * F * 4  # noqa: E731
    assert size(E.POLICY_S16) == 266_880_000 <= 256 << 20 < size(E.POLICY_S2) == 268_800_000
    assert round(size(139) / 2 ** 20, 1) == 254.5 and round(size(140) / 2 ** 20, 1) == 256.3
    p = E.pattern(N, W, F, False, E.POLICY_L)
    assert (p.m == E.POLICY_L).any() and (p.m < E.POLICY_L).any()


# ---------------------------------------------------------------- the fold
@pytest.mark.parametrize("shape", [s for s, _ in E.FOLD_FORMS], ids=lambda s: "x".join(map(str, s)))
def test_fold_ring_holds_the_chunk_boundaries(shape):
    N, W, F = shape
    c = E.fold_ring(N, W, F)
    la = c.bounds[0][1]
    assert la >= W + 1 + 210 and 0 < c.oldest < c.H and c.count == c.H
    st, env = E.fold_starts(c)
    assert len(st) == E.FOLD_S == len(set(st.tolist()))
    h0 = (c.oldest + st) % c.H
    last = (h0 + W - 1) % c.H + E.counts(c, st, env, 200) - 1
    assert (last >= c.H).any() and (last < c.H).any()                        # folds across the array's end, and not
    run = E.counts(c, st, env, 10 ** 6)
    for n in E.FOLD_N:
        m = E.counts(c, st, env, n)
        have = set(m.tolist())
        assert n in have and {v for v in (1, 63, 64, 65, 127, 128, 129) if v <= n} <= have, (n, have)
        cut = (m == run) & (m < n) & (st < la)                               # by the second episode's first row
        assert {v for v in (64, 65) if v < n} <= set(m[cut].tolist())
        for gamma in E.FOLD_GAMMA:
            e = E.fold_expect(N, W, F, n, gamma)
            assert np.array_equal(e.m, m)
            r = [c.rewards[(h0[j] + W - 1 + np.arange(m[j])) % c.H, env[j]] for j in range(len(st))]
            assert all((x > 0).any() and (x < 0).any() for x, mj in zip(r, m) if mj >= 63)   # mixed sign
            if gamma == 1.0:
                assert (e.disc == 1.0).all() and (np.abs(e.R - e.plain) <= E.fold_bound(e.plain, m, e.mag)).all()
                assert np.allclose(e.mag, [np.abs(x.astype(np.float64)).sum() for x in r], rtol=1e-12)


def test_fold_reference_is_the_horner_chain_of_the_nstep_test():
    c = E.fold_ring(3, 3, 3)
    R, fused, disc, mag = E.fold_ref(c, [c.oldest], [1], [3], 0.9)
    g = np.float64(np.float32(0.9))
    r = c.rewards[(c.oldest + 2 + np.arange(3)) % c.H, 1].astype(np.float64)
    assert R[0] == r[0] + g * (r[1] + g * r[2]) and disc[0] == g * g * g
    assert mag[0] == abs(r[0]) + abs(g * r[1]) + abs(g * g * r[2])
    assert abs(fused[0] - R[0]) <= 2 * np.spacing(abs(R[0]))                  # one rounding a step instead of two
    assert E.ulp32(1.0) == 2.0 ** -23 and E.ulp32(-3.0) == 2.0 ** -22
    assert E.fold_bound(1.0, 64, 10.0) == 2.0 ** -23 + 64 * 2.0 ** -52 * 10.0


# ---------------------------------------------------------------- generic forms, alignment
def test_generic_boundary_shapes_sit_on_the_boundaries():
    image = lambda N, D, F: N * D * F * 4  # noqa: E731
    assert image(64, 63 + 1, 4) == 65536 < image(64, 64 + 1, 4)              # one-step: W + 1 staged days
    assert image(64, 32 + 32, 4) == 65536 < image(64, 33 + 33, 4)            # n-step: W + min(n, W)
    assert 5 * 3 * 3 == 45 and 45 % 4                                        # the LDS kernels' scalar write-out
    assert (256 * 3 * 3) % 4 == 0                                            # .. and their 16-B write-out at N = 256
    assert E.GENERIC_S > 14                                                  # the candidates come round


def test_alignment_cases_move_the_right_pointers():
    assert E.ALIGN_OFFS == {2: (1, 0), 1: (0, 1), 0: (1, 1)}                 # bit 0: outputs aligned, bit 1: series
    for aligned, (out_off, series_off) in E.ALIGN_OFFS.items():
        assert bool(aligned & 1) == (out_off == 0) and bool(aligned & 2) == (series_off == 0)
