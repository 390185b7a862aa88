"""Measure pmenv_restart_days (per-env episodes on the resident series).

1. One restart call at the BASELINE shape (65,536 x 30 x 50 x 5) with k of the envs
   restarting, against the composition it replaces: pmenv_window_init_days for all envs
   into a scratch, a masked copy over the live window, pmenv_reset(mask).
2. step + restart against the step plus `day += 1` (what a lockstep loop does), with no env
   restarting and with B / 1,024 restarting per step, at the BASELINE shape (flat, in place)
   and at config 2 (4,096 x 30, relay, in place): the price of the call and of the
   unconditional re-prime of the flat / relay step's copies.

HIP events on the calling stream, one process, the two sides alternating (five rounds of
`--reps` groups of 10 back-to-back calls each); a side's time is the median of its rounds
and its spread (max - min) / median. Prints one JSON object; `--out` writes it too
(profiles/rows_restart.json).
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

from pmenv import MarketSeries, TradingEnv, _abi  # noqa: E402

FAR = 1 << 30
DAY0 = 200          # the bar every pinned env sits on


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


def both(new, old, reps, before=None):
    """(new us, new spread, old us, old spread), the sides alternating."""
    tn, to = [], []
    for _ in range(5):
        if before:
            before()
        tn.append(timeit(new, reps))
        if before:
            before()
        to.append(timeit(old, reps))
    n, o = statistics.median(tn), statistics.median(to)
    return n, (max(tn) - min(tn)) / n, o, (max(to) - min(to)) / o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _abi.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, W, F, T = 30, 50, 5, 2048
    g = torch.Generator(device=dev).manual_seed(0)
    bars = 100 * torch.exp(torch.cumsum(0.01 * torch.randn(T, N, 1, device=dev, generator=g), 0)).expand(T, N, 4)
    ms = MarketSeries(bars.contiguous(), device=dev)
    res = []

    def ck(rc, h, what):
        if rc:
            _abi.check(rc, h, what)

    def setup(B, impl, k):
        """A reset env of B envs with k of them (spread evenly) pinned:
        each sits on DAY0 with end = DAY0 + 1 and restart = DAY0 - W, so every restart call
        restarts exactly those k and leaves them on DAY0 again."""
        env = TradingEnv(num_envs=B, num_assets=N, window=W, features=F, device=dev, track_info=False,
                         step_impl=impl)
        start = torch.full((B,), DAY0 - W, dtype=torch.int32, device=dev)
        obs = ms.initial_window(start, W)
        env.reset(obs)
        sel = torch.zeros(B, dtype=torch.bool, device=dev)
        if k:
            sel[torch.arange(k, device=dev) * (B // k)] = True
        day0 = torch.full((B,), DAY0, dtype=torch.int32, device=dev)
        day = day0.clone()
        end = torch.where(sel, DAY0 + 1, FAR).to(torch.int32)
        done = torch.zeros(B, dtype=torch.uint8, device=dev)
        return env, obs, start, sel, day0, day, end, done

    # ---- 1. one restart call against the composition
    B = 65536
    for k in (0, 64, 4096, 65536):
        env, obs, restart, sel, day0, day, end, done = setup(B, "flat", k)
        scratch = torch.empty_like(obs)
        mask = sel.to(torch.uint8)
        m4 = sel.view(B, 1, 1, 1)

        def new():
            ck(lib.pmenv_restart_days(env._h, P(obs), P(ms.bars), T, P(day), P(end), P(restart), P(done), st),
               env._h, "pmenv_restart_days")

        def old():
            ck(lib.pmenv_window_init_days(P(scratch), P(ms.bars), T, N, F, P(restart), B, W, st), None,
               "pmenv_window_init_days")
            torch.where(m4, scratch, obs, out=obs)
            ck(lib.pmenv_reset(env._h, P(obs), P(mask), st), env._h, "pmenv_reset")

        n, ns, o, os_ = both(new, old, a.reps, before=lambda: day.copy_(day0))
        assert int(done.sum()) == k
        row = {"case": "restart_call", "B": B, "k": k, "restart_us": round(n, 2), "restart_spread": round(ns, 4),
               "composition_us": round(o, 2), "composition_spread": round(os_, 4), "ratio": round(n / o, 4),
               "faster_beyond_spreads": bool(o - n > ns * n + os_ * o),
               "bytes_restart": int(k * (N * W * F * 4 + N * W * 16 + N * W * 4) + 13 * B)}
        print(json.dumps(row), file=sys.stderr)
        res.append(row)
        env.close()
        del env, obs, scratch

    # ---- 2. the step with episodes against the step plus day += 1
    for name, B, impl in (("baseline_flat", 65536, "flat"), ("config2_relay", 4096, "relay")):
        for k in (0, B // 1024):
            env, obs, restart, sel, day0, day, end, done = setup(B, impl, k)
            act = torch.softmax(torch.randn(B, N, device=dev, generator=g), -1)
            rew = torch.empty(B, device=dev)
            args = _abi.PmenvStepArgs()
            args.action, args.bar, args.day, args.series_days = act.data_ptr(), ms.bars.data_ptr(), day.data_ptr(), T
            args.obs, args.reward = obs.data_ptr(), rew.data_ptr()

            def new():
                ck(lib.pmenv_step_ex(env._h, ctypes.byref(args), st), env._h, "pmenv_step_ex")
                ck(lib.pmenv_restart_days(env._h, P(obs), P(ms.bars), T, P(day), P(end), P(restart), P(done), st),
                   env._h, "pmenv_restart_days")

            def old():
                ck(lib.pmenv_step_ex(env._h, ctypes.byref(args), st), env._h, "pmenv_step_ex")
                day.add_(1)

            n, ns, o, os_ = both(new, old, a.reps, before=lambda: day.copy_(day0))
            row = {"case": "step_with_episodes", "shape": name, "B": B, "impl": impl, "restarting_per_step": k,
                   "step_restart_us": round(n, 2), "step_restart_spread": round(ns, 4),
                   "step_day_add_us": round(o, 2), "step_day_add_spread": round(os_, 4),
                   "extra_us": round(n - o, 2), "ratio": round(n / o, 4), "step_path": env.step_path}
            print(json.dumps(row), file=sys.stderr)
            res.append(row)
            env.close()
            del env, obs

    out = {"tool": "tools/bench_restart.py", "device": torch.cuda.get_device_name(dev), "reps": a.reps, "rows": res}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
