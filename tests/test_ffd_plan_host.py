"""The fractional-differencing plan (csrc/ffd_plan.h) on the CPU: the taps and widths of
pmenv_ffd_weights against the reference's own (tests/golden/ffd/ffd_*.npz, bit for bit), the
d = 1 and d = 0 cases, the refusals, and pmenv_ffd_path's name and geometry against a Python
transcription of the plan's rules over a sweep of (T, C, max_width). tests/host/
ffd_plan_sweep.cpp, a program that includes nothing but the header, is compiled with the
plain host C++ compiler — and once more under the address and undefined-behaviour
sanitizers, run as its own process — and must print what the library returns. Nothing here
touches a device."""
import ctypes
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from pmenv import _abi, features
from ffd_ref import golden, golden_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_SRC = os.path.join(ROOT, "tests", "host", "ffd_plan_sweep.cpp")
GOLDENS = (("mixed_t600", 600), ("t6000", 6000))
RB, JB, WAVES, CHUNK = 8, 8, 4, 256
I32_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------- the transcription
def plan(T, C, mw):
    if T < 1 or C < 1 or mw < 0 or mw >= T:
        return None
    cw = 16 if C <= 16 else 32 if C <= 32 else 64
    slots = 64 // cw
    rows = WAVES * slots * RB
    gx, gy = -(-(T - mw) // rows), -(-C // cw)
    if gx > I32_MAX or gy > 65535:
        return None
    return dict(cw=cw, slots=slots, rows=rows, grid=(gx, gy), block=64 * WAVES, rb=RB, jb=JB)


def expected(T, C, mw):
    p = plan(T, C, mw)
    if p is None:
        return ""
    return (f"ffd_apply_kernel<{RB},{JB}> cw={p['cw']} slots={p['slots']} rows={p['rows']} "
            f"grid={p['grid'][0]}x{p['grid'][1]} block={p['block']}")


def scale_expected(T, C):
    chunks = -(-T // CHUNK) if T >= 1 and C >= 1 else 0
    if chunks > 65535:
        chunks = 0
    return chunks, chunks * max(C, 0) * 16


TS = (1, 2, 31, 32, 33, 64, 65, 128, 129, 257, 400, 600, 6000, 12000, 1 << 20, I32_MAX)
CS = (1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 256, 2000, 65535 * 64, 65535 * 64 + 1, I32_MAX)
MWS = (0, 1, 7, 8, 9, 63, 64, 65, 926, 4075)


@functools.lru_cache(maxsize=None)
def plan_cases():
    cases = [(T, C, mw) for T, C, mw in itertools.product(TS, CS, MWS)]
    cases += [(T, C, T + k) for T, C in itertools.product((1, 2, 33, 400), (1, 64)) for k in (-1, 0, 1)]
    cases += [(0, 4, 0), (-1, 4, 0), (4, 0, 0), (4, -1, 0), (4, 4, -1), (-I32_MAX - 1, -I32_MAX - 1, -I32_MAX - 1)]
    return cases


def test_ffd_path_matches_the_transcribed_plan():
    lib = _abi.load()
    seen = set()
    for T, C, mw in plan_cases():
        got = lib.pmenv_ffd_path(T, C, mw).decode()
        assert got == expected(T, C, mw), (T, C, mw)
        seen.add(got.split(" grid=")[0])
    assert "" in seen and len(seen) == 4                          # refusals and the three wave shapes
    name, geo = features.ffd_path(12000, 256, 4000)
    assert name == "ffd_apply_kernel<8,8>" and geo == plan(12000, 256, 4000)
    assert features.ffd_path(10, 3, 10) == ("", {})


def test_scale_workspace_matches_the_transcription():
    lib = _abi.load()
    for T, C in itertools.product((0, 1, 2, 255, 256, 257, 1000, 12000, 65535 * 256, 65535 * 256 + 1, I32_MAX),
                                  (0, 1, 3, 64, 65, 2000)):
        assert lib.pmenv_scale_workspace(T, C) == scale_expected(T, C)[1], (T, C)


# ---------------------------------------------------------------- the weights
@pytest.mark.parametrize("name,T", GOLDENS)
def test_taps_and_widths_equal_the_reference_bit_for_bit(name, T):
    g = golden(name)
    for d, w, ref in zip(g["d"], g["widths"], golden_taps(g)):
        taps, width = features.ffd_weights(d, float(g["thres"]), T)
        assert width == w, (d, width, w)
        assert taps.dtype == np.float32 and np.array_equal(taps.view(np.uint32), ref.view(np.uint32)), d


def test_identity_leave_alone_and_refusals():
    taps, width = features.ffd_weights(1.0, 1e-5, 600)            # weights[:width] drops tap `width`: no first difference
    assert width == 1 and taps.tolist() == [1.0]
    taps, width = features.ffd_weights(0.0, 1e-5, 600)            # leave the column alone
    assert width == 0 and taps.size == 0
    taps, width = features.ffd_weights(2.0, 1e-5, 600)            # 1, -2, 1, 0, ...: width 2
    assert width == 2 and taps.tolist() == [1.0, -2.0]
    assert features.ffd_weights(0.5, 1e-5, 2)[1] == 1             # T - 1 taps at the most
    lib = _abi.load()
    w = ctypes.c_int32(7)
    for d, thres, T in ((-0.1, 1e-5, 600), (float("nan"), 1e-5, 600), (float("inf"), 1e-5, 600), (0.5, -1.0, 600),
                        (0.5, float("nan"), 600), (0.5, 1e-5, 1), (0.5, 1e-5, 0), (0.5, 1e-5, -3)):
        assert lib.pmenv_ffd_weights(d, thres, T, None, 0, ctypes.byref(w)) == -1, (d, thres, T)
    assert lib.pmenv_ffd_weights(0.5, 1e-5, 600, None, 0, None) == -1
    assert lib.pmenv_ffd_weights(0.5, 1e-5, 600, None, 4, ctypes.byref(w)) == -1   # cap without a buffer
    buf = (ctypes.c_float * 4)(9, 9, 9, 9)                        # cap < width: cap taps, the full width
    assert lib.pmenv_ffd_weights(0.5, 1e-5, 600, buf, 3, ctypes.byref(w)) == 0 and w.value > 3
    assert list(buf)[:3] == [1.0, -0.5, -0.125] and buf[3] == 9.0


def test_apply_refuses_a_filter_as_wide_as_the_series_before_any_launch():
    """max_width >= T is PMENV_ERR_ARG, as are overlapping ranges: decided on the host from
    the pointers' values (host buffers here: nothing is launched)."""
    lib = _abi.load()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    p = lambda off: ctypes.c_void_p(base + 4 * off)  # noqa: E731
    wid = (ctypes.c_int32 * 8)()
    for T, mw in ((10, 10), (10, 11), (1, 1), (0, 0), (10, -1)):
        assert lib.pmenv_ffd_apply(p(0), T, 4, p(1024), wid, mw, p(2048), None) == -1, (T, mw)
    assert lib.pmenv_ffd_apply(p(0), 10, 0, p(1024), wid, 2, p(2048), None) == -1
    assert lib.pmenv_ffd_apply(None, 10, 4, p(1024), wid, 2, p(2048), None) == -1
    # x is [10, 4] = 40 floats: out inside it, out one float into its end, the tap table under out
    assert lib.pmenv_ffd_apply(p(0), 10, 4, p(1024), wid, 2, p(0), None) == -1
    assert lib.pmenv_ffd_apply(p(0), 10, 4, p(1024), wid, 2, p(39), None) == -1
    assert lib.pmenv_ffd_apply(p(40), 10, 4, p(1024), wid, 2, p(9), None) == -1    # out [8, 4] ends inside x
    assert lib.pmenv_ffd_apply(p(0), 10, 4, p(1024), wid, 2, p(1024 + 7), None) == -1
    assert lib.pmenv_ffd_apply(ctypes.c_void_p(base + 2), 10, 4, p(1024), wid, 2, p(2048), None) == -4


# ---------------------------------------------------------------- the header on its own
def compile_sweep(tmp_path, name, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, SWEEP_SRC], check=True)
    return out


WEIGHT_CASES = [(d, th, T) for d in (0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0, 1.5, 2.0, 3.0)
                for th, T in ((1e-3, 600), (1e-5, 6000), (1e-2, 300), (0.0, 50), (2.0, 50))] + \
               [(-0.1, 1e-5, 600), (0.5, -1.0, 600), (0.5, 1e-5, 1), (0.5, 1e-5, 2), (0.5, 1e-5, -5), (1e-9, 1e-5, 100),
                (0.5, 1e-300, 20000)]


def library_lines():
    lib = _abi.load()
    out = []
    for d, th, T in WEIGHT_CASES:
        w = ctypes.c_int32(-1)
        rc = lib.pmenv_ffd_weights(d, th, T, None, 0, ctypes.byref(w))
        taps = np.zeros(max(w.value, 0) if rc == 0 else 0, dtype=np.float32)
        if taps.size:
            rc = lib.pmenv_ffd_weights(d, th, T, taps.ctypes.data_as(ctypes.c_void_p), taps.size, ctypes.byref(w))
        out.append(" ".join([str(rc), str(w.value)] + [f"{b:08x}" for b in taps.view(np.uint32)]))
    out += [lib.pmenv_ffd_path(T, C, mw).decode() for T, C, mw in plan_cases()]
    out += ["%d %d" % (scale_expected(T, C)[0], lib.pmenv_scale_workspace(T, C)) for T, C in SCALE_CASES]
    return out


SCALE_CASES = [(1, 1), (256, 64), (257, 65), (12000, 256), (65535 * 256 + 1, 4), (0, 4), (4, 0), (I32_MAX, I32_MAX)]


def run_sweep(binary):
    text = "".join(f"W {d!r} {th!r} {T}\n" for d, th, T in WEIGHT_CASES)
    text += "".join(f"P {T} {C} {mw}\n" for T, C, mw in plan_cases())
    text += "".join(f"S {T} {C}\n" for T, C in SCALE_CASES)
    r = subprocess.run([binary], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[-1] == ""
    return lines[:-1]


def test_header_compiles_without_hip_and_agrees_with_the_library(tmp_path):
    """The plain host compiler builds a program from ffd_plan.h alone (no HIP include path, no
    library), and it prints the library's taps, widths, paths and workspace sizes."""
    assert run_sweep(compile_sweep(tmp_path, "ffd_plan_sweep")) == library_lines()


def test_header_is_clean_under_the_sanitizers(tmp_path):
    """The same program under -fsanitize=address,undefined (the runtimes linked into it), as its
    own process: no report — the tap buffer holds exactly `width` floats — and the same lines."""
    binary = compile_sweep(tmp_path, "ffd_plan_sweep_san", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan")
    assert run_sweep(binary) == library_lines()
