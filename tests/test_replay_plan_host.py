"""The sample gathers' kernel choice (csrc/replay_plan.h) by name and geometry, on the CPU:
pmenv_replay_path with cus = 256 touches no device. The rules below are a Python
transcription of the four entry points as they chose their kernels inline before the plan
existed (one copy of the group search per gather, as they stood there), compared string for
string over a sweep of shapes; the anchors pin the shapes the GPU tests and the measured
rows rely on, and every name the sweep returns must be a kernel the library holds."""
import functools
import itertools
import re
import subprocess

from pmenv import _abi
from pmenv.replay import gather_path

CUS = 256
NS = (1, 2, 3, 4, 7, 8, 30, 61, 64, 122, 256, 257, 300, 512)
WS = (1, 2, 3, 4, 5, 8, 10, 49, 50)
FS = (3, 5, 8)
SS = (1, 16, 128, 700)
ALIGNED = (0, 1, 2, 3)                  # bit 0: outputs 16-B aligned, bit 1: series
KINDS = ("one_step", "nstep", "seq", "rollout")
U32 = 0xFFFFFFFF


def n_values(W):
    return sorted({1, 2, W, W + 1, 2 * W + 3, 64})


def ppt_ladder(pairs, top):
    if pairs <= 2 * 256:
        return 2
    if pairs <= 4 * 256:
        return 4
    if top == 8 or pairs <= 8 * 256:
        return 8
    return 12


def text(name, R, grid, lds, D=0, Lc=0, nc=0):
    return (f"{name} R={R}" + (f" D={D}" if D else "") + (f" Lc={Lc} nc={nc}" if Lc else "") +
            f" grid={grid[0]}x{grid[1]} lds={lds}")


@functools.lru_cache(maxsize=None)
def one_step_group(N, W, F):
    for r in range(N, 0, -1):
        if N % r == 0 and (r * W * F) % 4 == 0 and r * (W + 1) <= 2048 and r <= 256:
            return r
    return 0


def one_step(N, F, W, n, S, aligned, cus):
    out_al, ser_al = bool(aligned & 1), bool(aligned & 2)
    lds = N * (W + 1) * F * 4
    R = one_step_group(N, W, F) if F == 5 and out_al and ser_al else 0
    if R > 0:
        pairs, gy = R * (W + 1), N // R
        G = cus // gy if cus // gy > 0 else 1
        return text(f"replay_gather_f5p_kernel<{ppt_ladder(pairs, 8)},2>", R, (min(S, G), gy), R * (W + 1) * F * 4,
                    D=W + 1)
    if lds <= 64 * 1024 and N <= 256 and out_al:
        return text("replay_gather_lds_kernel", 0, (S, 1), lds, D=W + 1)
    return text("replay_gather_kernel", 0, (((S * N * W * F + 255) // 256) & U32, 1), 0)


@functools.lru_cache(maxsize=None)
def nstep_group(N, W, F, D):
    for r in range(N, 0, -1):
        if N % r == 0 and (r * W * F) % 4 == 0 and r * D <= 12 * 256 and r <= 256 and r * D * F * 4 <= 64 * 1024:
            return r
    return 0


def nstep(N, F, W, n, S, aligned, cus):
    out_al, ser_al = bool(aligned & 1), bool(aligned & 2)
    D = W + min(n, W)
    lds = N * D * F * 4
    R = nstep_group(N, W, F, D) if F == 5 and out_al and ser_al else 0
    if R > 0:
        pairs, gy = R * D, N // R
        G = cus // gy if cus // gy > 0 else 1
        return text(f"replay_nstep_f5p_kernel<{ppt_ladder(pairs, 12)},2>", R, (min(S, G), gy), R * D * F * 4, D=D)
    if lds <= 64 * 1024 and N <= 256 and out_al:
        return text("replay_nstep_lds_kernel", 0, (S, 1), lds, D=D)
    return text("replay_nstep_kernel", 0, (((S * N * W * F + 255) // 256) & U32, 1), 0)


@functools.lru_cache(maxsize=None)
def seq_group(N, W, F, lc):
    D = W + lc
    for r in range(min(N, 256), 0, -1):
        if N % r == 0 and (r * W * F) % 4 == 0 and r * D <= 12 * 256 and (r * D * F + 4) * 4 <= 64 * 1024:
            return r
    return 0


def seq(N, F, W, L, S, aligned, cus):
    R = 0
    if F == 5 and aligned == 3:
        R = seq_group(N, W, F, min(L, 8)) or seq_group(N, W, F, 1)
    gy = N // R if R else 1
    if R > 0 and S * gy * L <= 1 << 30:
        cap = min(12 * 256 // R, (64 * 1024 // 4 - 4) // (F * R)) - W
        cap = min(cap, 256, L)
        nc = (L + min(cap, 8) - 1) // min(cap, 8)
        want = (cus + S * gy - 1) // (S * gy)
        if nc < want:
            nc = min(want, L)
        Lc = (L + nc - 1) // nc
        nc = (L + Lc - 1) // Lc
        items = S * gy * nc
        D = W + Lc
        policy = 16 if S * L * N * W * F * 4 <= 256 << 20 else 2
        return text(f"replay_seq_f5p_kernel<{ppt_ladder(R * D, 12)},{policy}>", R, (min(items, cus), 1),
                    (R * D * F + 4) * 4, D=D, Lc=Lc, nc=nc)
    blocks = (S * L * N * W * F + 255) // 256
    if blocks > 0x7FFFFFFF:
        return ""
    return text("replay_seq_kernel", 0, (blocks, 1), 0)


def rollout(N, F, W, n, S, aligned, cus):
    lds = W * N * F * 4
    if F == 5 and (N * W * F) % 4 == 0 and lds <= 64 * 1024 and aligned == 3:
        small = S * N * W * F * 4 <= 128 << 20
        return text(f"rollout_gather_tile_kernel<{16 if small else 2}>", 0, (S, 1), lds)
    return text("rollout_gather_rows_kernel", 0, ((S * N + 3) // 4, 1), 0)


RULES = {"one_step": one_step, "nstep": nstep, "seq": seq, "rollout": rollout}


@functools.lru_cache(maxsize=None)
def sweep():
    """{(kind, N, W, F, n, S, aligned): pmenv_replay_path's answer} over the whole sweep."""
    lib = _abi.load()
    out = {}
    for kind, N, W, F, S, al in itertools.product(KINDS, NS, WS, FS, SS, ALIGNED):
        for n in n_values(W):
            out[kind, N, W, F, n, S, al] = lib.pmenv_replay_path(_abi.REPLAY_KINDS[kind], N, F, W, n, S, al,
                                                                 CUS).decode()
    return out


def test_replay_path_matches_the_transcribed_rules():
    got = sweep()
    assert len(got) >= 4 * 14 * 9 * 3 * 4 * 4 * 4
    for (kind, N, W, F, n, S, al), path in got.items():
        assert path == RULES[kind](N, F, W, n, S, al, CUS), (kind, N, W, F, n, S, al)
    forms = {(k[0], p.split("_kernel")[0]) for k, p in got.items()}
    assert forms == {("one_step", "replay_gather_f5p"), ("one_step", "replay_gather_lds"), ("one_step", "replay_gather"),
                     ("nstep", "replay_nstep_f5p"), ("nstep", "replay_nstep_lds"), ("nstep", "replay_nstep"),
                     ("seq", "replay_seq_f5p"), ("seq", "replay_seq"),
                     ("rollout", "rollout_gather_tile"), ("rollout", "rollout_gather_rows")}


def fields(path):
    name, *rest = path.split(" ")
    return name, dict(kv.split("=") for kv in rest)


def test_replay_path_anchors():
    """The shapes the rows in profiles/ were measured at and the forms the GPU tests rely on,
    worked out by hand from the rules."""
    p = functools.partial(gather_path, cus=CUS)
    assert p("one_step", 30, 50, S=8192) == "replay_gather_f5p_kernel<8,2> R=30 D=51 grid=256x1 lds=30600"
    assert p("nstep", 30, 50, n=5, S=8192) == "replay_nstep_f5p_kernel<8,2> R=30 D=55 grid=256x1 lds=33000"
    assert p("nstep", 30, 50, n=64, S=8192) == "replay_nstep_f5p_kernel<12,2> R=30 D=100 grid=256x1 lds=60000"
    assert fields(p("nstep", 64, 50, n=64, S=64))[1]["R"] == "16"
    assert p("seq", 30, 50, n=64, S=16) == "replay_seq_f5p_kernel<8,16> R=30 D=54 Lc=4 nc=16 grid=256x1 lds=32416"
    name, f = fields(p("seq", 30, 50, n=64, S=128))
    assert name == "replay_seq_f5p_kernel<8,16>" and (f["Lc"], f["nc"]) == ("8", "8")
    assert fields(p("seq", 64, 50, n=64, S=128))[0].endswith(",2>")          # above 256 MiB of windows: nt stores
    assert fields(p("one_step", 300, 50))[1]["R"] == "30"
    assert fields(p("nstep", 300, 50, n=1))[1]["R"] == "60"
    for kind, small, prime in (("one_step", "replay_gather_lds_kernel", "replay_gather_kernel"),
                               ("nstep", "replay_nstep_lds_kernel", "replay_nstep_kernel"),
                               ("seq", "replay_seq_kernel", "replay_seq_kernel"),
                               ("rollout", "rollout_gather_rows_kernel", "rollout_gather_rows_kernel")):
        assert fields(p(kind, 3, 3, F=3, n=2, S=64))[0] == small
        assert fields(p(kind, 257, 3, F=5, n=2, S=64))[0] == prime
    # 61 assets: no 16-B granular group, and the sample's 55 days are past the LDS form's 64 KiB
    assert fields(p("nstep", 61, 50, n=5, S=64))[0] == "replay_nstep_kernel"
    assert fields(p("rollout", 30, 50, S=4096))[0] == "rollout_gather_tile_kernel<16>"
    assert fields(p("rollout", 30, 50, S=32768))[0] == "rollout_gather_tile_kernel<2>"


def test_replay_path_rejects_bad_arguments():
    lib = _abi.load()
    ok = (0, 30, 5, 50, 1, 64, 3, CUS)
    assert lib.pmenv_replay_path(*ok) != b""
    for i, bad in ((0, 4), (0, -1), (1, 0), (2, 1), (3, 0), (5, 0), (6, 4), (6, -1)):
        assert lib.pmenv_replay_path(*ok[:i], bad, *ok[i + 1:]) == b"", (i, bad)
    assert lib.pmenv_replay_path(1, 30, 5, 50, 0, 64, 3, CUS) == b""          # the n-step gather's n < 1
    assert lib.pmenv_replay_path(2, 30, 5, 50, 0, 64, 3, CUS) == b""          # the sequence gather's L < 1
    assert lib.pmenv_replay_path(0, 30, 5, 50, 0, 64, 3, CUS) != b""          # n unused
    # a sequence gather past 2^31 - 1 workgroups of the element form: PMENV_ERR_ARG there, "" here
    assert lib.pmenv_replay_path(2, 2 ** 20, 3, 2 ** 10, 64, 2 ** 10, 3, CUS) == b""


def test_every_named_kernel_is_in_the_library():
    syms = subprocess.run(["nm", "-C", _abi.LIB_PATH], capture_output=True, text=True).stdout
    stubs = {m.replace(" ", "") for m in re.findall(r"__device_stub__(\w+(?:<[^>]*>)?)\(", syms)}
    assert stubs, "no kernel stubs found"
    names = {p.split(" ")[0] for p in sweep().values() if p}
    # every instantiation the product can launch but the nt tile (above 128 MiB of windows) and the
    # sequence gather's plain-store forms (the tools build's PMENV_SEQ_NT=0)
    assert len(names) == 22
    assert names <= stubs, f"named but not instantiated: {sorted(names - stubs)}"
