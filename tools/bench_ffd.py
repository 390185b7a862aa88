"""Feature-pipeline timings on the GPU: pmenv_ffd_apply, the column scalers and
features.build against the reference's own forms in torch, in one process.

    python tools/bench_ffd.py [--out profiles/rows_ffd.json] [--rounds 5] [--iters 5] [--quick]

Shapes: T = 12,000 rows (data_loader.py:34 keeps tickers with at least as many), thres =
1e-5, at N = 32, C = 8 (config/base.py:28-29 and the loader's default features) and at
N = 500, C = 4; d drawn from 0.1 .. 0.9 per column. Baselines, in torch on the same device:

    conv1d_loop      one conv1d per column over that column's own taps: ffd.py:85-87 as written
    conv1d_grouped   one grouped conv1d, every column padded to max_width (the strongest torch form)
    torch_minmax / torch_standard   amin / amax / mean / std plus the arithmetic

The candidates alternate within every round (A B A B ...), each timed with HIP events over
`iters` back-to-back calls after a warm-up; a row records the median over the rounds and the
spread (min .. max). The per-column loop is timed on 64 columns and scaled to all of them.
The conv1d forms compute in f32 with their own summation order; the kernel keeps one f64
chain per output (include/pmenv.h), so the rows compare cost, not bits.
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

from pmenv import features  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, iters):
    """microseconds per call over `iters` back-to-back calls between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(cands, rounds, iters):
    """{name: [us per round]}: every candidate once per round, in turn"""
    for fn in cands.values():           # warm-up: first-call work (kernel load, conv autotune) is not timed
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


def bench_shape(T, N, C, thres, rounds, iters, loop_cols=64, probe_s=20.0):
    rng = np.random.default_rng(N * 100 + C)
    cols = N * C
    d = np.round(rng.uniform(0.1, 0.9, (N, C)), 2)
    close = 50 * np.exp(np.cumsum(0.012 * rng.standard_normal((T + 1, N)), axis=0))
    raw = (close[:, :, None] * np.exp(0.003 * rng.standard_normal((T + 1, N, C)))).astype(np.float32)
    raw[..., min(3, C - 1)] = close
    x = torch.from_numpy(raw[1:].reshape(T, cols)).to(DEV)
    table, widths, mw = features.tap_table(d, thres, T, (N, C))
    tab, wd = torch.from_numpy(table).to(DEV), torch.from_numpy(widths).to(DEV)
    out = torch.empty(T - mw, cols, device=DEV)
    shape = dict(T=T, N=N, C=C, columns=cols, thres=thres, max_width=mw, width_min=int(widths.min()),
                 width_mean=round(float(widths.mean()), 1))
    name, geo = features.ffd_path(T, cols, mw)
    rows = []

    # the reference's form: per column, its own flipped taps, the last T - max_width outputs
    xt = x.t().contiguous()                                        # [cols, T]: a column is a contiguous sequence
    taps = [torch.from_numpy(table[:widths[c], c][::-1].copy()).to(DEV).reshape(1, 1, -1) for c in range(cols)]

    wpad = torch.zeros(cols, 1, mw, device=DEV)
    for c in range(cols):
        wpad[c, 0, mw - widths[c]:] = taps[c].reshape(-1)

    def conv_grouped():                                            # out[t] for t >= max_width - 1; drop the first
        return torch.nn.functional.conv1d(xt.unsqueeze(0), wpad, groups=cols)[0, :, 1:]

    def kernel():
        return features.ffd_apply(x, tab, wd, mw, out=out)

    got = kernel().clone()
    flops = 2.0 * float(widths.astype(np.int64).sum()) * (T - mw)
    t = alternate({"ffd_apply": kernel}, rounds, iters)
    med = sorted(t["ffd_apply"])[len(t["ffd_apply"]) // 2]
    rows.append(row("ffd_apply", shape, t["ffd_apply"], kernel=name, geometry=geo, gflops=round(flops / (med * 1e3), 1)))

    # a baseline's first call is probed by the wall clock (torch picks and may build its
    # convolution there): one that takes longer than `probe_s` is recorded by that call alone
    def probe(fn):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize(DEV)
        return res, time.perf_counter() - t0

    grouped, took = probe(conv_grouped)
    shape_g = dict(shape, first_call_s=round(took, 2),
                   vs_kernel_max_rel=float(((grouped.t() - got).abs() / (torch.abs(x[mw:]) + 1.0)).max()))
    del grouped
    if took <= probe_s:
        t = alternate({"ffd_apply": kernel, "conv1d_grouped": conv_grouped}, rounds, iters)
        rows.append(row("ffd_apply (beside conv1d_grouped)", shape, t["ffd_apply"]))
        rows.append(row("conv1d_grouped", shape_g, t["conv1d_grouped"]))
    else:
        rows.append(row("conv1d_grouped", shape_g, [took * 1e6], note="first call only: above the probe limit"))

    # the per-column loop on at most `loop_cols` columns, scaled to all of them (one launch
    # chain per column: the cost is linear in the columns)
    sub = min(cols, loop_cols)

    def conv_loop():
        res = torch.empty(sub, T - mw, device=DEV)
        for c in range(sub):
            res[c] = torch.nn.functional.conv1d(xt[c].reshape(1, 1, -1), taps[c]).reshape(-1)[-(T - mw):]
        return res

    _, took = probe(conv_loop)
    shape_l = dict(shape, columns_timed=sub, first_call_s=round(took, 2))
    if took <= probe_s:
        t = alternate({"conv1d_loop": conv_loop}, max(rounds // 2, 2), 1)
        rows.append(row("conv1d_loop", shape_l, [u * cols / sub for u in t["conv1d_loop"]],
                        note="timed on columns_timed columns, scaled to all"))
    else:
        rows.append(row("conv1d_loop", shape_l, [took * 1e6 * cols / sub], note="first call only: above the probe limit"))

    # the scalers on the differenced rows
    y = got
    buf = torch.empty_like(y)
    for method in ("minmax", "standard"):
        def ours(method=method):
            return features.scale(y, method, out=buf)

        def torch_form(method=method):
            if method == "minmax":
                lo, hi = y.amin(0), y.amax(0)
                den = hi - lo
                return (y - lo) / torch.where(den == 0, torch.ones_like(den), den)
            mean, std = y.mean(0), y.std(0, unbiased=False)
            return (y - mean) / torch.where(std == 0, torch.ones_like(std), std)

        t = alternate({f"scale_{method}": ours, f"torch_{method}": torch_form}, rounds, iters)
        rows.append(row(f"scale_{method}", shape, t[f"scale_{method}"], note="fit + apply, workspace allocated per call"))
        rows.append(row(f"torch_{method}", shape, t[f"torch_{method}"]))

    # the whole loader order, host-side tap tables included
    raw_d = torch.from_numpy(raw).to(DEV)
    t0 = time.perf_counter()
    features.build(raw_d, d, thres=thres)
    torch.cuda.synchronize(DEV)
    first = (time.perf_counter() - t0) * 1e6
    t = alternate({"build": lambda: features.build(raw_d, d, thres=thres)}, max(rounds // 2, 2), 1)
    rows.append(row("features.build", shape, t["build"], first_call_us=round(first, 1),
                    note="wall time dominated by the host-side weights (one per distinct d) and the table upload"))
    return rows


def dump(path, rows, a):
    """after every shape: a run cut short keeps what it measured"""
    rec = dict(tool="tools/bench_ffd.py", device=torch.cuda.get_device_name(DEV), rounds=a.rounds, iters=a.iters,
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_ffd.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="T = 3,000 and N = 8 / 40: a functional pass")
    a = ap.parse_args()
    torch.cuda.set_device(DEV)
    T = 3000 if a.quick else 12000
    shapes = ((8, 8), (40, 4)) if a.quick else ((32, 8), (500, 4))
    rows = []
    for N, C in shapes:
        rows += bench_shape(T, N, C, 1e-5, a.rounds, a.iters)
        dump(a.out, rows, a)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
