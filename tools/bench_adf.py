"""Timings of the search for the orders of differencing on the GPU: one pmenv_adf call and one
full find_d search at [5,000, 256] and [5,000, 2,000], beside what a user would write today,
in one process.

    python tools/bench_adf.py [--out profiles/rows_adf.json] [--rounds 5] [--iters 3] [--quick]

Rows per shape:

    pmenv_adf              one call on random-walk columns (the default lag rule: maxlag 32 at 5,000 rows)
    torch lstsq            the same regressions as batched torch.linalg.lstsq calls on the device in
                           f64: one per lag order 0 .. maxlag on the common rows, one final fit (the
                           statistic needs its residuals and the level's own regression on the other
                           columns), over the first 64 columns and scaled to the shape's columns (all
                           of them through it ran for minutes); a row records the error text if the
                           build's lstsq refuses the call
    numpy, per column      tests/adf_ref.py's adf() on the host over 16 columns, scaled to the shape's
                           columns (the reference's own way: one column after another)
    find_d                 the whole search: 16 rounds of table, FFD, ADF and update, the read-back
    numpy search           tests/adf_ref.py's search() on the host over 2 columns, scaled likewise

The device candidates alternate within every round, each timed with HIP events over `iters`
back-to-back calls (the lstsq form: one) after a warm-up; find_d is timed by the wall clock
around one synchronised call per round (it allocates its buffers and reads the result back,
as a user's call does). A row records the median over the rounds and the spread.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pm-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adf_ref  # noqa: E402
from pmenv import _abi, features  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(cands, rounds, iters):
    """cands: name -> (fn, iters or None for the default)"""
    for fn, _ in cands.values():
        fn()
    torch.cuda.synchronize(DEV)
    out = {k: [] for k in cands}
    for r in range(rounds):
        for k, (fn, it) in cands.items():
            out[k].append(timed(fn, it or iters))
        print(f"# round {r + 1}/{rounds}: " + ", ".join(f"{k} {v[-1]:.1f} us" for k, v in out.items()), flush=True)
    return out


def row(name, shape, us, **extra):
    us = sorted(us)
    r = dict(name=name, **shape, us_median=round(us[len(us) // 2], 2), us_min=round(us[0], 2), us_max=round(us[-1], 2),
             rounds=len(us), **extra)
    print(json.dumps(r), flush=True)
    return r


def walks(T, C):
    g = torch.Generator(device=DEV).manual_seed(T + C)
    return torch.cumsum(torch.randn(T, C, generator=g, device=DEV), 0).contiguous()


class TorchAdf:
    """adfuller's regressions as a user would batch them with torch.linalg.lstsq: the design
    [1, level, D_-1 .. D_-K] of every column at once in f64, one lstsq per lag order"""

    def __init__(self, x):
        T, C = x.shape
        self.K = adf_ref.maxlag_rule(T)
        x64 = x.to(torch.float64).t().contiguous()                         # [C, T]
        D = x64[:, 1:] - x64[:, :-1]
        K, nobs = self.K, T - 1 - self.K
        cols = [torch.ones(C, nobs, dtype=torch.float64, device=DEV), x64[:, K:T - 1]]
        cols += [D[:, K - j:T - 1 - j] for j in range(1, K + 1)]
        self.X = torch.stack(cols, dim=2).contiguous()                     # [C, nobs, K + 2]
        self.y = D[:, K:].unsqueeze(2).contiguous()
        self.nobs = nobs

    def __call__(self):
        X, y, K = self.X, self.y, self.K
        aic = []
        for k in range(K + 1):
            Xk = X[:, :, :k + 2]
            res = y - Xk @ torch.linalg.lstsq(Xk, y).solution
            aic.append(self.nobs * torch.log((res * res).sum((1, 2)) / self.nobs) + 2.0 * (k + 2))
        used = torch.stack(aic).argmin(0)
        # the final fit at the commonest lag stands for the per-column final fits (same cost)
        k = int(K // 2)
        Xk = X[:, :, :k + 2]
        beta = torch.linalg.lstsq(Xk, y).solution
        res = y - Xk @ beta
        others = torch.cat([Xk[:, :, :1], Xk[:, :, 2:]], dim=2)
        lvl = Xk[:, :, 1:2]
        rl = lvl - others @ torch.linalg.lstsq(others, lvl).solution
        stat = beta[:, 1, 0] / torch.sqrt((res * res).sum((1, 2)) / (self.nobs - k - 2) / (rl * rl).sum((1, 2)))
        return stat, used


def host_adf_us(x, cols):
    xs = x[:, :cols].cpu().numpy()
    t = time.perf_counter()
    for c in range(cols):
        adf_ref.adf(xs[:, c])
    return (time.perf_counter() - t) * 1e6 / cols


def host_search_us(x, cols, thres):
    xs = x[:, :cols].cpu().numpy()
    t = time.perf_counter()
    for c in range(cols):
        adf_ref.search(xs[:, c], thres, features.ffd_weights)
    return (time.perf_counter() - t) * 1e6 / cols


def dump(path, rows, a):
    rec = dict(tool="tools/bench_adf.py", device=torch.cuda.get_device_name(DEV), rounds=a.rounds, iters=a.iters,
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_adf.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="[600, 64] only: a functional pass")
    a = ap.parse_args()
    torch.cuda.set_device(DEV)
    _abi.load()
    rows = []
    for T, C in ((600, 64),) if a.quick else ((5000, 256), (5000, 2000)):
        shape = dict(T=T, C=C)
        x = walks(T, C)
        path = " | ".join(n + " " + " ".join(f"{k}={v}" for k, v in g.items()) for n, g in features.adf_path(T, C))
        out = features.adf(x)
        work = torch.empty(_abi.load().pmenv_adf_workspace(T, C, -1) // 8, dtype=torch.float64, device=DEV)
        cands = {"pmenv_adf": (lambda: features.adf(x, out=out, work=work), None)}
        t = alternate(cands, a.rounds, a.iters)                            # on its own first: a row whatever follows
        rows.append(row("pmenv_adf, alone", shape, t["pmenv_adf"], kernels=path,
                        usedlag_mean=round(float(out["usedlag"].float().mean()), 2)))
        dump(a.out, rows, a)
        err, sub = None, min(C, 64)
        try:
            ref = TorchAdf(x[:, :sub].contiguous())
            t0 = time.perf_counter()
            stat, used = ref()
            torch.cuda.synchronize(DEV)
            print(f"# torch lstsq, {sub} columns, first call: {time.perf_counter() - t0:.2f} s", flush=True)
            cands["torch lstsq"] = (ref, 1)
        except Exception as e:      # a build whose batched f64 lstsq is missing: recorded, not hidden
            err = f"{type(e).__name__}: {e}"[:200]
        t = alternate(cands, a.rounds, a.iters)
        rows.append(row("pmenv_adf", shape, t["pmenv_adf"], kernels=path))
        if err is None:
            agree = float((used.to(torch.int32) == out["usedlag"][:sub]).float().mean())
            rows.append(row("torch lstsq", shape, [v * C / sub for v in t["torch lstsq"]], columns_timed=sub,
                            lstsq_calls=ref.K + 3, usedlag_equal_share=round(agree, 4)))
        else:
            rows.append(dict(name="torch lstsq", **shape, error=err))
            print(json.dumps(rows[-1]), flush=True)
        print("# numpy, 16 columns on the host", flush=True)
        per = [host_adf_us(x, 16) for _ in range(2)]
        rows.append(row("numpy, per column", shape, [p * C for p in per], columns_timed=16, us_per_column=round(min(per), 1)))
        dump(a.out, rows, a)

        wall = []
        for _ in range(a.rounds + 1):
            torch.cuda.synchronize(DEV)
            t0 = time.perf_counter()
            d, info = features.find_d(x)
            wall.append((time.perf_counter() - t0) * 1e6)
            print(f"# find_d: {wall[-1] / 1e3:.1f} ms", flush=True)
        rows.append(row("find_d", shape, wall[1:], evals_mean=round(float(info["evals"].mean()), 2),
                        d_mean=round(float(d.mean()), 4), width_max=int(info["width"].max())))
        per = [host_search_us(x, 2, 1e-5)]
        rows.append(row("numpy search", shape, [p * C for p in per], columns_timed=2, us_per_column=round(per[0], 1)))
        dump(a.out, rows, a)
        del x, out, work, cands
        torch.cuda.empty_cache()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
