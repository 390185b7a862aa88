"""The step's shape plan (csrc/step_plan.h) by kernel name and geometry, on the CPU:
pmenv_step_path_for touches no device. The rules below are a Python transcription of the
plan as it stood inline in pmenv_create_in, handle.h's helpers, the four *_bits functions of
pmenv_set_step_path and pmenv_step_path before the header existed, compared string for
string over a sweep of shapes that sits one env either side of every byte threshold; the
anchors pin the shapes the GPU tests assert and the BASELINE configs DESIGN.md §3 records.
tests/host/step_plan_sweep.cpp, a program that includes nothing but the header, is compiled
with the plain host C++ compiler — and once more under the address and undefined-behaviour
sanitizers, run as its own process — and must print what the library returns."""
import ctypes
import functools
import itertools
import os
import shutil
import subprocess

import pytest

from pmenv import _abi, step_path_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_SRC = os.path.join(ROOT, "tests", "host", "step_plan_sweep.cpp")

NS = (1, 5, 8, 16, 17, 30, 32, 33, 64, 65, 100, 128, 129, 256, 500, 512, 513)
WS = (1, 2, 3, 13, 14, 32, 50)
FS = (2, 3, 4, 5, 8, 9, 12, 16, 17)
COMMISSIONS = (0.0, 0.0025)
PATHS = (0, 1, 2, 3, 4)                 # auto, one_launch, two_launch, flat, relay
MIB = 1 << 20
THRESHOLDS = tuple(m * MIB for m in (2, 16, 24, 48, 100, 128, 192, 256, 1024))
I32_MAX = 2 ** 31 - 1
DB, IP = 1, 2                           # PMENV_FUSE_DB, PMENV_FUSE_INPLACE
K1STR = 100000
TILE_FLOATS = 8192


# ---------------------------------------------------------------- the transcription
def scratch_bytes(tile_floats, N, F):
    return tile_floats * 4 + N * 16 + N * 8 + N * (F - 1) * 4 + 16


def plan_streaming(N, W, F, order):
    WF = W * F
    if F != 5 or (N * WF) % 4:
        return None
    align = 1
    while (align * WF) % 4:
        align += 1
    for V in order:
        cap = 512 * 4 * V
        R = cap // WF
        R = N if R >= N else R - R % align
        if R < 1 or R * WF > cap:
            continue
        return R, V
    return None


def pick_k1_vec(B, N):
    if B * N * 4 >= 1 << 32:
        return 0
    for top, v in ((8, 801), (16, 1601), (64, None), (128, 6402), (256, 6404), (512, 6408)):
        if N <= top:
            return K1STR + v if v else 0
    return 0


@functools.lru_cache(maxsize=None)
def plan(B, N, W, F, commission):
    """The handle's plan fields as pmenv_create_in left them; None where it refused the cfg."""
    if B < 1 or N < 1 or W < 1 or F < 2 or not 0.0 <= commission < 1.0:
        return None
    WF = W * F
    if WF > TILE_FLOATS or N * WF >= 1 << 31:
        return None
    p = {}
    R = min(TILE_FLOATS // WF, N)
    vec = (N * WF) % 4 == 0
    if vec and R < N:
        while R > 0 and (R * WF) % 4:
            R -= 1
        if R == 0:
            vec, R = False, TILE_FLOATS // WF
    p["rows_per_tile"], p["vec"] = R, vec
    nwf = N * WF
    p["small_block"] = 256 if nwf <= 256 * 16 else 512 if nwf <= 512 * 16 else 1024 if nwf <= 1024 * 16 else 0
    p["small_e"] = 8 if nwf <= 256 * 8 else 16
    p["tiny"] = p["small_block"] == 256 and p["small_e"] == 8 and N <= 64 and N * (F - 1) <= 2 * 256
    per = N * W * F
    win = B * per * 4
    surf_lds = (4 * 1024 // WF + 2) * (W + 1) * 4
    p["surf_stream"] = (win > 256 * MIB and nwf % 4 == 0 and B * (nwf // 4) < (1 << 31) - 1024 and
                        surf_lds <= 64 << 10 and 4 * 1024 // WF + 2 <= 256)
    tile_floats = (R * WF + 3) // 4 * 4
    lds_tile = scratch_bytes(tile_floats, N, F)

    ip, db = plan_streaming(N, W, F, (2, 4, 1)), plan_streaming(N, W, F, (4, 2, 1))
    streaming = p["streaming"] = ip is not None and db is not None
    flat_ok = streaming and F == 5 and W >= 2 and per % 4 == 0 and B * (per // 4) < (1 << 31) - 1024
    p["flat"] = p["flat_inplace"] = flat_ok
    p["flat_ip_block"], p["flat_ip_vec"] = (256 if win <= 256 * MIB else 512), 2
    p["flat_pol"] = 0 if win <= 128 * MIB else 1
    p["flat_ip_pol"] = 0 if win <= 256 * MIB else 1
    k1 = p["k1_vec"] = pick_k1_vec(B, N)
    per4 = per // 4

    # the one-workgroup-per-env step, 4 chunks per lane
    blocks = (per4 + 126) // 64
    one_waves = p["one_waves"] = (blocks + 3) // 4
    one_ok = p["one_ok"] = (streaming and F == 5 and W >= 2 and N <= 64 and per % 4 == 0 and one_waves <= 16 and
                            (64 * 4 * one_waves + 2) * 16 <= 65536)
    one_auto = DB | IP if one_ok and (win <= 48 * MIB or not flat_ok) else 0

    # the flat one-launch step
    def flat1_fits(block, v):
        cpw = block * v
        ne_max = (cpw + per4 - 2) // per4 + 1 if per4 else 0
        span_rows = (4 * cpw - 1) // WF + 2
        wide_ok = N <= 512 and span_rows <= 64
        return flat_ok and (N <= 64 or wide_ok) and ne_max <= block // 64
    band128 = N <= 64 and 1023 <= per4 < 2000 and win > 1 << 30
    if band128 and flat1_fits(128, 8):
        fb, fv = 128, 8
    elif flat1_fits(256, 4):
        fb, fv = 256, 4
    else:
        fb, fv = 512, 2
    p["flat1_block"], p["flat1_vec"] = fb, fv
    flat1_ok = p["flat1_ok"] = flat1_fits(fb, fv) and (N <= 64 or fb == 256)
    flat1_auto = 0
    if flat1_ok and N <= 64 and fb <= 256 and per4 >= 1000:
        if win > 48 * MIB:
            flat1_auto |= DB
        if win > 256 * MIB:
            flat1_auto |= IP
        one_auto &= ~flat1_auto
    if flat1_ok and 64 < N <= 128 and win > 1 << 30 and not commission > 0.0:
        flat1_auto |= IP
    one_fill = per4 / (256.0 * one_waves) if one_ok else 0.0
    if 24 * MIB < win <= 100 * MIB:
        if one_ok and one_fill >= 0.9:
            one_auto |= IP
        elif flat1_ok and N <= 64:
            flat1_auto |= IP
            one_auto &= ~IP
        elif one_ok:
            one_auto |= IP

    # the relayed one-launch step
    kv = k1 - K1STR if k1 >= K1STR else k1
    rb, rv = p["flat_ip_block"], 2
    rows_fit = 4 * rb * rv // (W * 5) + 2 <= rb
    relay_ok = p["relay_ok"] = flat_ok and W >= 2 and rows_fit and N <= 512 and (N <= 64 or k1 != 0)
    kl = kv // 100 if kv else (32 if N <= 32 else 64)
    ka = kv % 100 if kv else 0
    relay_auto = 0
    if relay_ok and N <= 64:
        one_holds = one_ok and one_fill >= 0.9 and win <= 48 * MIB
        if 24 * MIB < win <= 256 * MIB and not one_holds:
            relay_auto |= IP
        if 48 * MIB < win <= 128 * MIB:
            relay_auto |= DB
        one_auto &= ~relay_auto
        flat1_auto &= ~relay_auto
        rows_fit4 = 4 * 256 * 4 // (W * 5) + 2 <= 256
        if relay_auto & IP and win > 192 * MIB and rb == 256 and kl == 32 and ka == 0 and rows_fit4:
            rv = 4
    p["relay_block"], p["relay_v"], p["relay_kl"], p["relay_ka"] = rb, rv, kl, ka

    # the generic stream
    p["gen_block"], p["gen_v"] = (512 if win > 128 * MIB else 256), 2
    gen_ok = p["gen_ok"] = (F != 5 and 2 <= F <= 16 and per % 4 == 0 and B * (per // 4) < (1 << 31) - 1024 and
                            4 * 1024 // WF + 2 <= 256)
    gen_auto = DB | IP if gen_ok and win > (16 * MIB if p["tiny"] else 2 * MIB) else 0

    p["one_auto"], p["flat1_auto"], p["relay_auto"], p["gen_auto"] = one_auto, flat1_auto, relay_auto, gen_auto
    # what follows the plan: the limits
    units = max((N + ip[0] - 1) // ip[0], (N + db[0] - 1) // db[0]) if streaming else 1
    scalar_scratch_floats = (scratch_bytes(0, N, F) // 4 + 3) // 4 * 4
    if lds_tile > 160 * 1024 or 4 * scalar_scratch_floats * 4 > 160 * 1024:
        return None
    if B * units >= 1 << 31:
        return None
    return p


def select(p, path):
    """pmenv_set_step_path's one_bits / flat1_bits / relay_bits / gen_bits; None where it refused."""
    both = DB | IP
    if path == 1:
        one = both if p["one_ok"] else -1
    elif path == 2:
        one = 0 if p["streaming"] or p["gen_ok"] else -1
    elif path == 3:
        one = 0 if p["flat1_ok"] else -1
    elif path == 4:
        one = 0 if p["relay_ok"] else -1
    else:
        one = p["one_auto"]
    flat1 = (both if p["flat1_ok"] else -1) if path == 3 else p["flat1_auto"] if path == 0 else 0
    relay = (both if p["relay_ok"] else -1) if path == 4 else p["relay_auto"] if path == 0 else 0
    gen = (both if p["gen_ok"] else 0) if path == 2 else p["gen_auto"] if path == 0 else 0
    if one < 0 or flat1 < 0 or relay < 0:
        return None
    return one, flat1, relay, gen


def names(p, N, sel):
    """pmenv_step_path's string for a handle that was never captured."""
    one, flat1, relay, gen = sel
    k1 = "scalar_step_vec_kernel" if p["k1_vec"] else "scalar_step_reg_kernel" if N <= 64 else "scalar_step_kernel"
    if not p["streaming"]:
        single = "step_tiny_kernel" if p["tiny"] else "step_small_kernel" if p["small_block"] else \
            "step_advance_lds_kernel"
        if not gen:
            return single
        g2 = k1 + "+advance_gen_kernel"
        return f"{g2 if gen & DB else single} (obs_out) | {g2 if gen & IP else single} (in place)"
    part = []
    for bit in (DB, IP):
        if relay & bit:
            part.append("step_relay_kernel")
        elif flat1 & bit:
            part.append("step_flat_vec_kernel" if N > 64 else "step_flat_kernel")
        elif one & bit:
            part.append("step_env_kernel")
        elif bit == DB:
            part.append(k1 + "+" + ("advance_flat_wg_kernel" if p["flat"] else "advance_rows_kernel"))
        else:
            part.append(k1 + "+" + ("advance_flat_inplace_kernel" if p["flat_inplace"] else "advance_rows_kernel"))
    return f"{part[0]} (obs_out) | {part[1]} (in place)"


def geometry(p, N):
    k1 = p["k1_vec"]
    kv = k1 - K1STR if k1 >= K1STR else k1
    k1s = f"{kv // 100}x{kv % 100}{'s' if k1 >= K1STR else ''}" if kv else ("reg" if N <= 64 else "lds")
    return (f"flat1={p['flat1_block']}x{p['flat1_vec']} "
            f"relay={p['relay_block']}x{p['relay_v']}:{p['relay_kl']}/{p['relay_ka']} "
            f"stream_ip={p['flat_ip_block']}x{p['flat_ip_vec']} pol={p['flat_pol']}/{p['flat_ip_pol']} "
            f"gen={p['gen_block']}x{p['gen_v']} k1={k1s} one_waves={p['one_waves']} "
            f"small={p['small_block']}x{p['small_e']} tiny={int(p['tiny'])} surf_stream={int(p['surf_stream'])} "
            f"rows_per_tile={p['rows_per_tile']} vec={int(p['vec'])}")


def expected(B, N, W, F, commission, path, detail=True):
    p = plan(B, N, W, F, commission)
    sel = select(p, path) if p else None
    if sel is None:
        return ""
    return names(p, N, sel) + (" -- " + geometry(p, N) if detail else "")


# ---------------------------------------------------------------- the sweep
def env_counts(N, W, F):
    """B = 1, one env below and one above every byte threshold of the rules, and the envs at
    the 2^31-chunk, 2^32-byte [B, N] descriptor and 2^31-workgroup limits."""
    per = N * W * F
    out = {1, I32_MAX}
    for t in THRESHOLDS:
        out |= {t // (per * 4), t // (per * 4) + 1}
    q = max(per // 4, 1)
    out |= {((1 << 31) - 1024) // q + d for d in (-1, 0, 1)}
    out |= {(1 << 30) // N + d for d in (-1, 0, 1)}               # B N 4 = 2^32
    units = -(-N // max(512 * 4 // (W * F), 1))                   # about the row stream's units per env
    out |= {(1 << 31) // units + d for d in (-1, 0, 1)}
    return sorted(b for b in out if 1 <= b <= I32_MAX)


@functools.lru_cache(maxsize=None)
def shapes():
    out = [(B, N, W, F) for N, W, F in itertools.product(NS, WS, FS) for B in env_counts(N, W, F)]
    assert len(out) >= 17 * 7 * 9 * 20
    return out


# cfgs out to the edge of int32, with products past 32 and 64 bits; the last block is refused outright
EXTREMES = ([(I32_MAX, N, W, F) for N, W, F in ((1, 1, 2), (1, 4096, 2), (1000, 1, 2), (4000, 1, 2), (5000, 4096, 2),
                                                 (262143, 4096, 2), (30, 50, 5), (5851, 1, 2), (5852, 1, 2),
                                                 (I32_MAX, 1, 2), (1, I32_MAX, 2), (1, 1, I32_MAX),
                                                 (I32_MAX, I32_MAX, I32_MAX), (65536, 8192, 2), (46341, 46341, 2))] +
            [(B, N, 50, 5) for B, N in ((65536, 32768), (1 << 20, 4096), (1 << 24, 512), (1 << 27, 8), (1 << 28, 4))] +
            [(0, 30, 50, 5), (-1, 30, 50, 5), (4, 0, 50, 5), (4, 30, 0, 5), (4, 30, 50, 1), (4, 30, 4000, 5),
             (-I32_MAX - 1, -I32_MAX - 1, -I32_MAX - 1, -I32_MAX - 1)])


def cfg_of(B, N, W, F, commission):
    c = _abi.PmenvCfg()
    _abi.load().pmenv_cfg_default(ctypes.byref(c), B, N, W, F)
    c.commission = commission
    return c


def library(cases):
    lib = _abi.load()
    return [lib.pmenv_step_path_for(ctypes.byref(cfg_of(B, N, W, F, cm)), path, 1).decode()
            for B, N, W, F, cm, path in cases]


@functools.lru_cache(maxsize=None)
def sweep_cases():
    cases = [(B, N, W, F, cm, path) for (B, N, W, F), cm, path in itertools.product(shapes(), COMMISSIONS, PATHS)]
    cases += [(B, N, W, F, cm, path) for (B, N, W, F), cm, path in itertools.product(EXTREMES, COMMISSIONS, PATHS)]
    return cases


@functools.lru_cache(maxsize=None)
def sweep():
    return library(sweep_cases())


def test_step_path_for_matches_the_transcribed_plan():
    got = sweep()
    seen = set()
    for case, path in zip(sweep_cases(), got):
        assert path == expected(*case), case
        seen.add(path.split(" -- ")[0])
    assert "" in seen                                            # refusals are compared too
    kernels = {k for s in seen for part in s.split(" | ") for k in part.split(" (")[0].split("+") if k}
    assert kernels == {"step_flat_kernel", "step_flat_vec_kernel", "step_relay_kernel", "step_env_kernel",
                       "scalar_step_vec_kernel", "scalar_step_reg_kernel", "scalar_step_kernel",
                       "advance_flat_wg_kernel", "advance_flat_inplace_kernel", "advance_rows_kernel",
                       "advance_gen_kernel", "step_tiny_kernel", "step_small_kernel", "step_advance_lds_kernel"}


def test_step_path_for_without_detail_and_bad_arguments():
    lib = _abi.load()
    for case in sweep_cases()[::97]:
        B, N, W, F, cm, path = case
        assert lib.pmenv_step_path_for(ctypes.byref(cfg_of(B, N, W, F, cm)), path, 0).decode() == \
            expected(*case, detail=False), case
    c = cfg_of(64, 30, 50, 5, 0.0)
    assert lib.pmenv_step_path_for(None, 0, 0) == b""
    assert lib.pmenv_step_path_for(ctypes.byref(c), -1, 0) == b"" and lib.pmenv_step_path_for(ctypes.byref(c), 5, 0) == b""
    for field, bad in (("close_channel", 4), ("close_channel", -1), ("reward_kind", 4), ("norm_mode", 2),
                       ("ring_mode", -1), ("ret_mode", 3), ("mu_max_iter", -1), ("commission", 1.0),
                       ("commission", -0.1), ("commission", float("nan"))):
        c = cfg_of(64, 30, 50, 5, 0.0)
        setattr(c, field, bad)
        assert lib.pmenv_step_path_for(ctypes.byref(c), 0, 1) == b"", (field, bad)
    c = cfg_of(64, 30, 50, 5, 0.0)
    c.ret_mode = 2                                               # AUTO is resolved at create: no refusal
    assert lib.pmenv_step_path_for(ctypes.byref(c), 0, 0) != b""


def split(path):
    head, _, geo = path.partition(" -- ")
    return head, dict(kv.split("=") for kv in geo.split(" "))


def auto(B, N, W=50, F=5, impl="auto", **kw):
    return split(step_path_for(num_envs=B, num_assets=N, window=W, features=F, step_impl=impl, detail=True, **kw))


def modes(head):
    db, ip = head.split(" | ")
    return db.split(" (")[0], ip.split(" (")[0]


def test_baseline_configs_as_design_records_them():
    """names and geometry of BASELINE configs 1-5."""
    head, g = auto(65536, 30)                                    # the BASELINE shape: 128 x 8, nt, both modes
    assert modes(head) == ("step_flat_kernel", "step_flat_kernel") and g["flat1"] == "128x8" and g["pol"] == "1/1"
    head, g = auto(16384, 30)
    assert modes(head) == ("step_flat_kernel", "step_flat_kernel") and g["flat1"] == "256x4"
    head, g = auto(8192, 30)                                     # config 4's 8-GPU share
    assert modes(head)[1] == "step_relay_kernel" and g["relay"] == "256x4:32/0"
    head, g = auto(4096, 30)                                     # config 2
    assert modes(head) == ("step_relay_kernel", "step_relay_kernel") and g["relay"] == "256x2:32/0"
    head, g = auto(8192, 500)                                    # config 5: two launches
    assert modes(head) == ("scalar_step_vec_kernel+advance_flat_wg_kernel",
                           "scalar_step_vec_kernel+advance_flat_inplace_kernel") and g["k1"] == "64x8s"
    head, g = auto(1, 5)                                         # config 1
    assert head == "step_tiny_kernel" and g["tiny"] == "1" and g["small"] == "256x8"
    head, g = auto(65536, 30, F=12, close_channel=10)
    assert modes(head) == ("scalar_step_reg_kernel+advance_gen_kernel",) * 2 and g["gen"] == "512x2"


def test_shapes_the_gpu_tests_assert():
    """test_gpu_auto_path_rule, test_gpu_flat_path_rules and test_gpu_generic_stream_auto_at_size."""
    def m(B, N, **kw):
        return modes(auto(B, N, **kw)[0])
    assert m(800, 8) == ("step_env_kernel", "step_env_kernel")                      # 6 MB
    assert m(1500, 30) == ("step_env_kernel", "step_env_kernel")                    # 45 MB
    assert m(1700, 30) == ("step_relay_kernel", "step_relay_kernel")                # 51 MB
    assert m(3000, 30) == ("step_relay_kernel", "step_relay_kernel")                # 90 MB
    assert m(4096, 30) == ("step_relay_kernel", "step_relay_kernel")                # 123 MB
    assert m(8192, 30) == ("step_flat_kernel", "step_relay_kernel")                 # 246 MB
    assert m(4096, 16)[1] == "step_relay_kernel"                                    # 66 MB, 78 % fill
    assert m(4096, 8) == ("step_env_kernel", "step_relay_kernel")                   # 33 MB, 65 % fill
    assert m(9000, 30) == ("step_flat_kernel", "step_flat_kernel")                  # 270 MB
    assert m(9000, 8) == ("step_relay_kernel", "step_relay_kernel")                 # 72 MB, 500 chunks per env
    assert m(18000, 8) == ("scalar_step_vec_kernel+advance_flat_wg_kernel", "step_relay_kernel")   # 144 MB
    assert "step_flat_kernel" not in auto(2000, 65)[0]                              # N > 64
    assert m(9000, 30, commission=0.0025) == ("step_flat_kernel", "step_flat_kernel")
    assert "step_flat_kernel" not in auto(9000, 30, commission=0.0025, impl="two_launch")[0]
    db, ip = m(16384, 100)                                                          # 1.6 GB
    assert ip == "step_flat_vec_kernel" and not db.startswith("step_flat")
    assert "step_flat" not in auto(8192, 500)[0]
    head, g = auto(5, 30, impl="flat")
    assert head == "step_flat_kernel (obs_out) | step_flat_kernel (in place)" and g["flat1"] == "256x4"
    for n, w in ((1, 4), (4, 20), (65, 50)):                                        # 5 / 100 chunks per env; N > 64
        assert step_path_for(num_envs=5, num_assets=n, window=w, step_impl="flat") == ""
        assert step_path_for(num_envs=5, num_assets=n, window=w) != ""
    for F in (8, 12, 16):
        head, g = auto(600, 30, F=F, commission=0.0025, reward="diff_sharpe", close_channel=F - 2)
        assert head.count("advance_gen_kernel") == 2 and g["gen"] == "256x2"
    with pytest.raises(ValueError):
        step_path_for(num_envs=4, step_impl="fastest")


# ---------------------------------------------------------------- the header on its own
def compile_sweep(tmp_path, name, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, SWEEP_SRC], check=True)
    return out


def run_sweep(binary, cases):
    text = "".join(f"{B} {N} {W} {F} {cm!r} {path}\n" for B, N, W, F, cm, path in cases)
    r = subprocess.run([binary], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[-1] == "" and len(lines) == len(cases) + 1
    return lines[:-1]


def test_header_compiles_without_hip_and_agrees_with_the_library(tmp_path):
    """The plain host compiler builds a program from step_plan.h alone (no HIP include path,
    no library), and over the whole sweep it prints what libpmenv.so returns."""
    binary = compile_sweep(tmp_path, "step_plan_sweep")
    assert run_sweep(binary, sweep_cases()) == sweep()


def test_header_is_clean_under_the_sanitizers(tmp_path):
    """The same program under -fsanitize=address,undefined (the runtimes linked into it), as its
    own process, on the sweep and on cfgs out to INT32_MAX in every dimension (products past 32
    and 64 bits): no report, and the library's and the transcription's accept / reject."""
    binary = compile_sweep(tmp_path, "step_plan_sweep_san", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan")
    got = run_sweep(binary, sweep_cases())
    assert got == sweep()
    extreme = [(*shape, cm, path) for shape, cm, path in itertools.product(EXTREMES, COMMISSIONS, PATHS)]
    for case, line in zip(extreme, run_sweep(binary, extreme)):
        B, N, W, F, cm, path = case
        assert (line != "") == (expected(B, N, W, F, cm, path) != ""), case
