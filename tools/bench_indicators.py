"""Indicator-stage timings on the GPU: pmenv_ind_apply over all eleven indicators at their
TA-Lib defaults, each form of the recurrences at the same shape, in one process.

    python tools/bench_indicators.py [--out profiles/rows_indicators.json] [--rounds 5] [--iters 3]
                                     [--envs 65536] [--quick]

Shapes: T = 5,000, N = 510, C = 5 (the reference's own: about 500 tickers x 5,000 rows) and
T = 306, N = envs x 30, C = 5 (a slice of the per-env synthetic series). Rows:

    all eleven ops         the call as the plan dispatches it (pmenv_ind_path's kernels)
    recurrences, seq/split the eight recurrence ops alone in each form — the tools library
                           (tools/libpmenv_ab.so) reads PMENV_IND_FORM; the product has no knob —
                           at the reference shape and over a sweep of N at T = 5,000, which is
                           what sets ind_plan.h's kIndSplitMaxCols
    windowed               bbands, stoch and cci alone
    copy                   a device-to-device copy of 2 GiB in the same process: the chip's copy
                           rate beside which the sequential form's bytes/s are read (its bytes:
                           the bars once plus the outputs once)

The candidates alternate within every round, each timed with HIP events over `iters`
back-to-back calls after a warm-up; a row records the median over the rounds and the spread.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pm-rl_amd"))

from pmenv import _abi, features  # noqa: E402

DEV = torch.device("cuda:0")
ALL = [(n, {}) for n in ("ema", "bbands", "macd", "atr", "rsi", "adx", "dx", "stoch", "cci", "obv", "adosc")]
SCANS = [(n, p) for n, p in ALL if n not in ("bbands", "stoch", "cci")]
WINDOWED = [(n, p) for n, p in ALL if n in ("bbands", "stoch", "cci")]


def bind(path):
    lib = ctypes.CDLL(path)
    for name, res, args in _abi.SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(cands, rounds, iters):
    for fn in cands.values():
        fn()
        fn()
    torch.cuda.synchronize(DEV)
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            out[k].append(timed(fn, iters))
    return out


def row(name, shape, us, **extra):
    us = sorted(us)
    r = dict(name=name, **shape, us_median=round(us[len(us) // 2], 2), us_min=round(us[0], 2), us_max=round(us[-1], 2),
             rounds=len(us), **extra)
    print(json.dumps(r), flush=True)
    return r


def bars_of(T, N):
    """a positive OHLCV random walk on the device"""
    g = torch.Generator(device=DEV).manual_seed(T + N)
    bars = torch.empty(T, N, 5, device=DEV)
    close = torch.exp(torch.cumsum(torch.randn(T, N, generator=g, device=DEV) * 0.015, 0)) * 50.0
    bars[..., 3] = close
    bars[..., 0] = close * 1.001
    bars[..., 1] = close * 1.01
    bars[..., 2] = close * 0.99
    bars[..., 4] = torch.randint(1, 2 ** 24, (T, N), generator=g, device=DEV).float()
    return bars


class Call:
    """one pmenv_ind_apply call of `lib` on preallocated buffers; form: None (the plan's rule), 0 or 1"""

    def __init__(self, lib, bars, spec, form=None, pool=None):
        self.lib, self.bars, self.form = lib, bars, form
        self.ops, _ = features.indicator_ops(spec)
        self.K, self.L, _ = features.indicator_layout(spec)
        self.T, self.N, self.C = bars.shape
        self.chan = (ctypes.c_int32 * 5)(0, 1, 2, 3, 4)
        self._knob(True)
        self.nbytes = lib.pmenv_ind_workspace(self.T, self.N, self.ops, len(self.ops))
        self.path = lib.pmenv_ind_path(self.T, self.N, self.ops, len(self.ops)).decode()
        self._knob(False)
        if pool is None:                                             # pool: (out floats, work doubles) shared by calls
            pool = (torch.empty((self.T - self.L) * self.N * self.K, device=DEV),
                    torch.empty(self.nbytes // 8 + 1, dtype=torch.float64, device=DEV))
        self.work = pool[1]
        self.out = pool[0][:(self.T - self.L) * self.N * self.K].view(self.T - self.L, self.N, self.K)
        assert self.work.numel() * 8 >= self.nbytes

    def _knob(self, on):
        if self.form is not None:
            if on:
                os.environ["PMENV_IND_FORM"] = str(self.form)
            else:
                os.environ.pop("PMENV_IND_FORM", None)

    def __call__(self):
        self._knob(True)
        rc = self.lib.pmenv_ind_apply(ctypes.c_void_p(self.bars.data_ptr()), self.T, self.N, self.C, self.chan, self.ops,
                                      len(self.ops), ctypes.c_void_p(self.out.data_ptr()), self.K, 0,
                                      ctypes.c_void_p(self.work.data_ptr()), self.nbytes,
                                      ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        self._knob(False)
        assert rc == 0, rc

    def bytes(self):
        """the bars once and the outputs once"""
        return 4 * (self.bars.numel() + self.out.numel())


def forms_at(ab, T, N, rounds, iters, rows, copy_tbs):
    bars = bars_of(T, N)
    shape = dict(T=T, N=N, C=5)
    seq, split = Call(ab, bars, SCANS, 0), Call(ab, bars, SCANS, 1)
    t = alternate({"seq": seq, "split": split}, rounds, iters)
    split()
    a = split.out.clone()
    seq()
    torch.cuda.synchronize(DEV)
    same = float((a.view(torch.int32) == seq.out.view(torch.int32)).float().mean())
    for k, c in (("seq", seq), ("split", split)):
        med = sorted(t[k])[len(t[k]) // 2]
        tbs = c.bytes() / (med * 1e-6) / 1e12
        rows.append(row(f"recurrences, {k}", shape, t[k], kernels=c.path, tb_per_s=round(tbs, 3),
                        of_copy_rate=round(tbs / copy_tbs, 3), bits_equal_share=round(same, 7)))
    del bars, seq, split, a
    torch.cuda.empty_cache()


def dump(path, rows, a):
    rec = dict(tool="tools/bench_indicators.py", device=torch.cuda.get_device_name(DEV), rounds=a.rounds, iters=a.iters,
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_indicators.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--envs", type=int, default=65536, help="envs of the per-env shape: N = envs x 30")
    ap.add_argument("--quick", action="store_true", help="T = 1,000 / N = 64 and 2,048 envs: a functional pass")
    a = ap.parse_args()
    torch.cuda.set_device(DEV)
    lib = _abi.load()
    ab = bind(os.path.join(ROOT, "tools", "libpmenv_ab.so"))
    rows = []

    n = 1 << 29                                                      # 2 GiB of floats
    src, dst = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    src.normal_()
    t = alternate({"copy": lambda: dst.copy_(src)}, a.rounds, a.iters)
    med = sorted(t["copy"])[len(t["copy"]) // 2]
    copy_tbs = 8.0 * n / (med * 1e-6) / 1e12
    rows.append(row("copy 2 GiB", {}, t["copy"], tb_per_s=round(copy_tbs, 3)))
    del src, dst
    torch.cuda.empty_cache()

    T_ref, N_ref = (1000, 64) if a.quick else (5000, 510)
    envs = 2048 if a.quick else a.envs
    for T, N in ((T_ref, N_ref), (306, envs * 30)):
        bars = bars_of(T, N)
        shape = dict(T=T, N=N, C=5)
        first = Call(lib, bars, ALL)                                 # the largest output and workspace: shared
        pool = (first.out.view(-1), first.work)
        calls = {"all eleven ops": first, "recurrences": Call(lib, bars, SCANS, pool=pool),
                 "windowed": Call(lib, bars, WINDOWED, pool=pool)}
        t = alternate(calls, a.rounds, a.iters)
        for k, c in calls.items():
            med = sorted(t[k])[len(t[k]) // 2]
            tbs = c.bytes() / (med * 1e-6) / 1e12
            rows.append(row(k, shape, t[k], kernels=c.path, tb_per_s=round(tbs, 3), of_copy_rate=round(tbs / copy_tbs, 3)))
        del bars, calls, first, pool
        torch.cuda.empty_cache()
        dump(a.out, rows, a)

    # both forms of the recurrences at one shape: the reference's, then more and more columns
    sweep = (64, 512) if a.quick else (510, 2048, 4096, 8192, 16384, 32768, 65536)
    for N in sweep:
        forms_at(ab, T_ref, N, a.rounds, a.iters, rows, copy_tbs)
        dump(a.out, rows, a)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
