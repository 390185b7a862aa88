"""Measure pmenv_metrics_episodes (per-episode trajectory metrics) against pmenv_metrics.

At the DESIGN.md §7 shape (T 252 x B 65,536 x N 30), three sides:
  1. pmenv_metrics, the lockstep kernel (unchanged);
  2. pmenv_metrics_episodes with dones = 0 and K = 1: the same 2.2 GB plus one done byte
     per (step, env), read by both of its parts;
  3. pmenv_metrics_episodes with per-env episodes of 64 - 200 rows (each env its own
     length and phase) and K = 5.

HIP events on the calling stream, one process, the three sides alternating (five rounds of
`--reps` groups of 10 back-to-back calls each); a side's time is the median of its rounds
and its spread (max - min) / median. Prints one JSON object; `--out` writes it too
(profiles/rows_metrics_env.json).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pm-rl_amd"))
import torch  # noqa: E402

from pmenv import _abi  # noqa: E402


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timeit(fn, reps, warmup=3, inner=10):
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(inner):
            fn()
        b.record(st)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--T", type=int, default=252)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _abi.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    T, B, N = a.T, a.B, a.N
    g = torch.Generator(device=dev).manual_seed(0)
    ret = 0.01 * torch.randn(T, B, dtype=torch.float64, device=dev, generator=g)
    val = torch.cat([torch.ones(1, B, dtype=torch.float64, device=dev), torch.cumprod(1.0 + ret, 0)])
    w = torch.softmax(torch.randn(T + 1, B, N, device=dev, generator=g), -1)
    none = torch.zeros(T, B, dtype=torch.uint8, device=dev)
    # env b ends an episode every L[b] rows, L in [64, 200], from its own phase
    L = torch.randint(64, 201, (B,), device=dev, generator=g)
    ph = (torch.rand(B, device=dev, generator=g) * L).long()
    t = torch.arange(T, device=dev).view(T, 1)
    eps = (((t + ph) % L) == L - 1).to(torch.uint8).contiguous()
    out1 = torch.empty(B, 5, dtype=torch.float64, device=dev)

    def bufs(K):
        return (torch.empty(B, K, 5, dtype=torch.float64, device=dev),
                torch.empty(B, K, 2, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))

    o2, o3 = bufs(1), bufs(5)

    def ck(rc, what):
        if rc:
            _abi.check(rc, None, what)

    def lockstep():
        ck(lib.pmenv_metrics(P(ret), P(val), P(w), T, B, N, 0.04, 252.0, P(out1), st), "pmenv_metrics")

    def episodes(d, K, o):
        def fn():
            ck(lib.pmenv_metrics_episodes(P(ret), P(val), P(w), P(d), T, B, N, 1.0, 0.04, 252.0, K, P(o[0]), P(o[1]),
                                          P(o[2]), st), "pmenv_metrics_episodes")
        return fn

    sides = [("pmenv_metrics", lockstep), ("episodes_dones0_K1", episodes(none, 1, o2)),
             ("episodes_64_200_K5", episodes(eps, 5, o3))]
    times = {name: [] for name, _ in sides}
    for _ in range(5):
        for name, fn in sides:
            times[name].append(timeit(fn, a.reps))
    torch.cuda.synchronize()
    assert int(o2[2].min()) == int(o2[2].max()) == 1
    assert torch.equal(o2[0][:, 0, 4], out1[:, 4])               # the final value: a copy on both sides
    cnt = o3[2]
    assert int(cnt.max()) <= 5 and int(cnt.min()) >= 2
    nbytes = T * B * 8 + (T + 1) * B * 8 + (T + 1) * B * N * 4
    rows = []
    for name, _ in sides:
        ts = times[name]
        m = statistics.median(ts)
        rows.append({"side": name, "us": round(m, 2), "spread": round((max(ts) - min(ts)) / m, 4),
                     "rounds_us": [round(x, 2) for x in ts], "GBps_of_inputs": round(nbytes / m / 1e3, 1)})
    base, zero = rows[0], rows[1]
    res = {"tool": "tools/bench_metrics_env.py", "device": torch.cuda.get_device_name(dev), "reps": a.reps,
           "T": T, "B": B, "N": N, "input_bytes": nbytes, "done_bytes": T * B,
           "episodes_per_env_mean": round(float(cnt.double().mean()), 3), "rows": rows,
           "dones0_over_lockstep": round(zero["us"] / base["us"], 4),
           "dones0_slower_beyond_spreads": bool(zero["us"] - base["us"] > zero["spread"] * zero["us"] +
                                                base["spread"] * base["us"])}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
