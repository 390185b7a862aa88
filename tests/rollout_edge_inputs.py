"""Edge-case rollouts for the GAE kernels and trajectories for the metrics kernel.

Deterministic generators that both the HIP kernels and the CPU restatement (oracle/) consume.
Env b takes class (b + shift) % K, so lane neighbours always differ. The GAE classes place
episode ends on the boundaries of every way the kernels of rollout.h cut the horizon: the
tile kernel's segments (counted from the end, seg_end = T, T - S, ...), the look-back
kernel's chunks (counted from day 0), the waves' sub-chunks of U days and the scan kernel's
lane chunks of L = ceil(T / 64) days. test_rollout_edges_host.py pins the generator's
preconditions and the case tables; test_gpu_rollout_edges.py drives the kernels with them.
"""
import numpy as np

# ------------------------------------------------------------------------------- GAE


def _cls_none(t, T, rng):
    return np.zeros(T, bool)


def _scan_chunk(t, T):
    L = (T + 63) // 64
    return (t % L == 0) | (t % L == L - 1)


DONE_CLASSES = [
    ("none", _cls_none),
    ("every", lambda t, T, rng: np.ones(T, bool)),
    ("last", lambda t, T, rng: t == T - 1),
    ("first", lambda t, T, rng: t == 0),
    ("mid", lambda t, T, rng: t == T // 2),
    ("c64_end", lambda t, T, rng: t % 64 == 63),              # look-back chunks, from day 0
    ("c64_start", lambda t, T, rng: t % 64 == 0),
    ("e64_end", lambda t, T, rng: (T - 1 - t) % 64 == 0),     # tile segments, from the end
    ("e64_start", lambda t, T, rng: (T - 1 - t) % 64 == 63),
    ("e128_end", lambda t, T, rng: (T - 1 - t) % 128 == 0),
    ("e128_start", lambda t, T, rng: (T - 1 - t) % 128 == 127),
    ("c128_end", lambda t, T, rng: t % 128 == 127),
    ("c128_start", lambda t, T, rng: t % 128 == 0),
    ("u8_end", lambda t, T, rng: t % 8 == 7),                 # wave sub-chunks
    ("u16_end", lambda t, T, rng: t % 16 == 15),
    ("scan_chunk", lambda t, T, rng: _scan_chunk(t, T)),      # first and last day of a lane chunk
    ("whole_chunk", lambda t, T, rng: (t >= 64) & (t < 128)),  # a map with C = 0 throughout
    ("iid", lambda t, T, rng: rng.random(T) < 0.02),
]
K = len(DONE_CLASSES)
CLASS = {name: i for i, (name, _) in enumerate(DONE_CLASSES)}


def done_class(b, shift=0):
    return (b + shift) % K


def gae_batch(T, B, seed, shift=0):
    """r [T, B] f32, v [T + 1, B] f32 (bootstrap row last), dones [T, B] uint8 (0 / 1); env b
    takes done class (b + shift) % K (shift: which class env 0 takes, for shapes with B < K)."""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((T, B)).astype(np.float32)
    v = rng.standard_normal((T + 1, B)).astype(np.float32)
    t = np.arange(T)
    pat = np.stack([f(t, T, rng) for _, f in DONE_CLASSES], 1).astype(np.uint8)      # [T, K]
    cls = (np.arange(B) + shift) % K
    d = np.ascontiguousarray(pat[:, cls])
    iid = np.flatnonzero(cls == CLASS["iid"])             # every i.i.d. env draws its own days
    d[:, iid] = rng.random((T, iid.size)) < 0.02
    return r, v, d


def stamp_done_bytes(dones):
    """A copy with every set byte replaced by one of 2, 128, 255 in turn: any non-zero byte
    is an episode end."""
    d = dones.copy()
    idx = np.flatnonzero(d)
    d.reshape(-1)[idx] = np.array([2, 128, 255], np.uint8)[np.arange(idx.size) % 3]
    return d


POISON_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def poison(r, v, what, t0, b0, value):
    """Copies of (r, v) with one element of `what` ('r' or 'v') set to a non-finite value
    (v's row T is the bootstrap row)."""
    r2, v2 = r.copy(), v.copy()
    (r2 if what == "r" else v2)[t0, b0] = POISON_VALUES[value] if isinstance(value, str) else value
    return r2, v2


def pieces(T, S, from_end):
    """[(first day, last day)] of the pieces a kernel cuts [0, T) into: S days from day 0
    (look-back chunks, wave sub-chunks of a chunk) or from the end (tile segments)."""
    if from_end:
        return [(max(e - S, 0), e - 1) for e in range(T, 0, -S)]
    return [(s, min(s + S, T) - 1) for s in range(0, T, S)]


def scan_pieces(T):
    L = (T + 63) // 64
    return [(min(l * L, T), min(l * L + L, T) - 1) for l in range(64) if min(l * L, T) < T]


def delta_exact(r, v, d, gamma):
    """f32(r + gamma (1 - d) v' - v) and f32(that + v) in numpy f64, gamma as the f32 the ABI takes:
    adv and ret wherever gamma * lambda * (1 - done) = 0."""
    g = float(np.float32(gamma))
    n = (d == 0).astype(np.float64)
    v64 = v.astype(np.float64)
    dl = r.astype(np.float64) + g * n * v64[1:] - v64[:-1]
    return dl.astype(np.float32), (dl + v64[:-1]).astype(np.float32)


def chunked_gae(r, v, d, gamma, lam, NW, U, from_end):
    """numpy f64 emulation of the chunked composition (not the kernels' code): every chunk of
    S = NW x U days is cut into NW wave sub-chunks, each reduced to its affine map (C, D); the
    chunk's map folds the waves' maps from wave NW - 1 down; the carry into a chunk composes the
    later chunks' maps sequentially, and every wave re-walks its days. Returns (adv, ret) f32."""
    T, B = r.shape
    g, gl = float(np.float32(gamma)), float(np.float32(gamma)) * float(np.float32(lam))
    n = (d == 0).astype(np.float64)
    v64 = v.astype(np.float64)
    dl = r.astype(np.float64) + g * n * v64[1:] - v64[:-1]
    c = gl * n
    S = NW * U
    chunks = pieces(T, S, from_end)                    # latest first when from_end
    if not from_end:
        chunks = chunks[::-1]
    adv = np.empty((T, B))
    carry = np.zeros(B)                                # advantage just after the chunk
    for s0, s1 in chunks:
        waves = [(s0 + w * U, min(s0 + w * U + U, s1 + 1)) for w in range(NW)]
        maps = []
        for a0, a1 in waves:
            C, D = np.ones(B), np.zeros(B)
            for t in range(a1 - 1, a0 - 1, -1):
                D = dl[t] + c[t] * D
                C = c[t] * C
            maps.append((C, D))
        for w, (a0, a1) in enumerate(waves):
            a = carry
            for j in range(NW - 1, w, -1):
                a = maps[j][1] + maps[j][0] * a
            for t in range(a1 - 1, a0 - 1, -1):
                a = dl[t] + c[t] * a
                adv[t] = a
        Ca, Da = np.ones(B), np.zeros(B)               # the chunk's map, folded from wave NW - 1
        for C, D in reversed(maps):
            Da = D + C * Da
            Ca = C * Ca
        carry = Da + Ca * carry
    return adv.astype(np.float32), (adv + v64[:-1]).astype(np.float32)


def compare_gae(got, ref, what=""):
    """The finite criterion: every element within one f32 ulp of the reference plus 1e-11 x its
    column's max |ref|, and at most 1 + 1e-5 T B elements not bit-equal. Both sides are f64
    recursions rounded once to f32: reassociation moves the f64 value by <~ T 2^-53 of the
    column scale, which flips a share ~3e-8 of the f32 roundings; an f32 intermediate flips
    tens of percent. Returns the number of differing elements."""
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    T, B = ref.shape
    col = np.abs(ref.astype(np.float64)).max(0, keepdims=True)
    tol = np.spacing(np.abs(ref)).astype(np.float64) + 1e-11 * col
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bad = ~(err <= tol)
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements beyond one ulp, first at "
                           f"{tuple(np.argwhere(bad)[0])}: {got[bad][0]!r} vs {ref[bad][0]!r}")
    ndiff = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    cap = 1 + 1e-5 * T * B
    assert ndiff <= cap, f"{what}: {ndiff} elements not bit-equal (cap {cap:.1f})"
    return ndiff


# --------------------------------------------------------------------------- metrics
METRIC_CLASSES = ["noise", "constant", "zero", "positive", "first_day", "rising", "falling", "peak_first",
                  "seg_peaks", "alt_weights"]
KM = len(METRIC_CLASSES)
MCLASS = {name: i for i, name in enumerate(METRIC_CLASSES)}
CONST_RET = 2.0 ** -7               # exact in every sum of the shapes used


def metrics_batch(T, B, N, seed):
    """returns [T, B] f64 (simple returns), values [T + 1, B] f64, weights [T + 1, B, N] f32;
    env b takes class b % KM. Return classes build values = cumprod(1 + returns); value classes
    set the values and derive the returns."""
    rng = np.random.default_rng(seed)
    ret = 0.01 * rng.standard_normal((T, B))
    val = np.empty((T + 1, B))
    z = rng.standard_normal((T + 1, B, N))
    e = np.exp(z - z.max(-1, keepdims=True))
    w = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    t1 = np.arange(T + 1, dtype=np.float64)
    for b in range(B):
        c = METRIC_CLASSES[b % KM]
        vb = None
        if c == "constant":
            ret[:, b] = CONST_RET
        elif c == "zero":
            ret[:, b] = 0.0
        elif c == "positive":
            ret[:, b] = np.abs(ret[:, b]) + 1e-4
        elif c == "first_day":
            ret[:, b] *= 0.1
            ret[0, b] = 1.0
        elif c == "rising":
            vb = 1.0 + 0.01 * t1
        elif c == "falling":
            vb = 1.0 / (1.0 + 0.01 * t1)
        elif c == "peak_first":      # peak on the first day, trough on the last: first and last wave segment
            vb = 1.0 + 0.05 * rng.random(T + 1)
            vb[0], vb[T] = 2.0, 0.5
        elif c == "seg_peaks":       # a new peak exactly on each wave segment's first day
            vb = 1.0 + 0.05 * rng.random(T + 1)
            for k in range(4):
                vb[(T + 1) * k // 4] = 2.0 + k
        elif c == "alt_weights":
            w[1::2, b] = w[1, b]
            w[0::2, b] = w[0, b]
        if vb is None:
            val[:, b] = np.concatenate([[1.0], np.cumprod(1.0 + ret[:, b])])
        else:
            val[:, b] = vb
            ret[:, b] = vb[1:] / vb[:-1] - 1.0
    return ret, val, w


def alt_turnover(w, b):
    """Closed-form average turnover of an alternating-weights env: T sum |w1 - w0| / T."""
    return np.abs(w[1, b].astype(np.float64) - w[0, b].astype(np.float64)).sum()


# ------------------------------------------------------------------------ case tables
TILE16, TILE8, TILE8_OCC8 = "gae_tile_kernel<8,16,1,2>", "gae_tile_kernel<8,8>", "gae_tile_kernel<8,8,8,2>"
SCAN, LOOP, LB8, LB16 = "gae_scan_kernel", "gae_kernel", "gae_lookback_kernel<8,8>", "gae_lookback_kernel<8,16>"

# (kernel, through, T, B, shift): the smallest shapes that reach each kernel and its boundaries.
# through: "gae" = rollout.gae (pmenv_gae_ex with a workspace), "direct" = pmenv_gae through
# the raw ABI. shift: env 0's done class where B < K leaves classes out.
GAE_CASES = [
    (TILE16, "gae", 1, 1, CLASS["every"]), (TILE16, "gae", 127, 1, CLASS["e64_end"]), (TILE16, "gae", 128, 65, 0),
    (TILE16, "gae", 129, 64, 0), (TILE16, "gae", 300, 130, 0),
    (TILE16, "direct", 1100, 70, 0), (TILE16, "direct", 640, 64, 0),      # many segments x few envs
    (TILE8, "gae", 65, 16384, 0), (TILE8, "gae", 130, 16385, 0),
    (TILE8_OCC8, "gae", 257, 65537, 0),
    (SCAN, "gae", 256, 1, CLASS["mid"]), (SCAN, "gae", 257, 63, 0),  # (257, 63): lanes >= 52 own no day
    (SCAN, "gae", 449, 3, CLASS["scan_chunk"]), (SCAN, "gae", 511, 5, CLASS["u16_end"]),
    (SCAN, "direct", 4097, 2, CLASS["scan_chunk"]),
    (LB8, "gae", 512, 1, CLASS["c64_end"]), (LB8, "gae", 513, 65, 0), (LB8, "gae", 577, 64, 0),
    (LB8, "gae", 700, 67, 0),
    (LB16, "gae", 1025, 900, 0), (LB16, "gae", 2048, 449, 0),
]
LOOP_CASES = [(37, 130, 0), (300, 5, CLASS["mid"])]          # tools build, PMENV_GAE=loop
FALLBACK_CASES = [(513, 3, CLASS["c64_end"]), (700, 67, 0), (1025, 900, 0)]   # tools build, PMENV_GAE=lbfb
GAMMA_LAMBDA = [(0.99, 0.95), (0.99, 1.0), (1.0, 1.0), (0.99, 0.0), (0.0, 0.95)]
# one shape per product kernel row for the non-finite leg (the two tools-build rows run it at
# LOOP_CASES and FALLBACK_CASES)
POISON_CASES = [(TILE16, "gae", 300, 130, 0), (TILE16, "direct", 640, 64, 0), (TILE8, "gae", 65, 16384, 0),
                (TILE8_OCC8, "gae", 257, 65537, 0), (SCAN, "gae", 257, 63, 0), (SCAN, "direct", 4097, 2, 0),
                (LB8, "gae", 700, 67, 0), (LB16, "gae", 1025, 900, 0)]

# kernel -> (S, counted from the end) of its segments / chunks
GEOMETRY = {TILE16: (128, True), TILE8: (64, True), TILE8_OCC8: (64, True), LB8: (64, False), LB16: (128, False)}

# (T, B, workspace) -> kernel: the selection rule as the tests rely on it
PATH_TABLE = [(T, B, through == "gae", k) for k, through, T, B, _ in GAE_CASES] + [
    (512, 1, False, SCAN), (513, 65, False, TILE16), (1025, 900, False, TILE16), (2048, 449, False, TILE16),
    (511, 8191, True, TILE16), (512, 8191, True, LB16), (512, 8192, True, TILE16), (512, 64, True, LB8),
    (255, 63, True, TILE16), (256, 63, True, SCAN), (256, 64, True, TILE16), (255, 65536, True, TILE8),
    (256, 65535, True, TILE8), (256, 65536, True, TILE8_OCC8), (64, 16383, True, TILE16), (64, 16384, True, TILE8),
    # (T + 1) B 4 bytes at 2^31: past the tile's and the look-back's buffer offsets
    (1, (1 << 28) - 1, True, TILE8), (1, 1 << 28, True, LOOP), (1 << 20, 511, True, LB16),
    (1 << 20, 512, True, LOOP), (1 << 20, 512, False, LOOP), (1 << 20, 63, False, SCAN), (1 << 25, 63, True, SCAN),
    (37, 130, True, TILE16), (300, 5, True, SCAN),
]

METRIC_SHAPES = [(1, 70, 3), (2, 5, 1), (3, 65, 30), (4, 64, 255), (6, 9, 256), (7, 130, 257), (64, 129, 30)]
METRIC_RATES = [(0.04, 252.0), (0.0, 252.0), (0.04, 12.0), (0.0, 12.0)]
