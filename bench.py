#!/usr/bin/env python
"""bench.py — whole-job env-steps/s of the fused portfolio-env step on MI355X.

One step = one pass of pmenv's fused env step over every env of the rank:
price relatives from the close channel, action normalisation, portfolio value
(f64), log-return reward, weight drift, and the one-day advance of the
[B, N, W, F] observation window.

Workload (BASELINE.json metric "env-steps/sec (whole node) at 65k envs x 30
assets"): 65,536 envs x 30 assets x 50-day window x 5 channels per GPU, synthetic
Philox OHLC series and softmax actions already resident in HBM. By default the
window is advanced in place — the reference's contract: step() mutates the
caller's features and returns them (trading_env.py:102-105); the double-buffered
advance (obs -> a fresh buffer, the form the device rollout buffer uses) is timed
as well and reported under "alt". `step_path` names the kernels one step launches.

Legs, in order (one process per GPU):
  1. lead-in, every rank: 64 steps of the bench's own workload through the same
     handle and buffers that are then timed. It carries the GPU past its start-up
     clock transient (profiles/warm_curve_r02a.json: steps 3-25 of a cold process
     run up to 1.3x slower), so the timed steps start at steady state whatever
     --warmup is. With --full it is also the parity leg: the first S envs' rewards
     and values are kept and, after the timed region, checked against the CPU
     restatement on the same inputs.
  2. --warmup untimed steps, then exactly --steps timed steps between barriers and
     device synchronisations; max over ranks.
  3. --dump-outputs DIR: what the last timed step handed its caller, as DIR/<name>.npy.
  4. --full only: the other window mode (alt), the collective (N > 1), the parity
     check, then on rank 0 at N = 1 the CPU baseline and the replay of the
     reference's own recorded outputs.

A plain run (no --full) stops after leg 3 and prints the result line with the keys
of legs 4 set to null; the headline (value, ms_per_step, roofline) is the same
measurement either way.

Multi-GPU runs are strong-scaled by default: the north star's 65,536 envs in total,
sharded over the ranks by global id (BASELINE config 4: 8,192 per GPU at N = 8; no
collective in the step); --global-envs G sets the total, --weak keeps 65,536 envs per
rank instead:

    python bench.py                                   # N = 1, the headline alone
    python bench.py --full                            # + alt, parity, CPU baseline, reference replay
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0. Refuses to run when any PMENV_* environment
variable is set (the product library reads none; nothing may alter the timed path).
"""
import argparse
import ctypes
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "pm-rl_amd"))

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec (MI355X_MICROARCH.md, Chip-level parameters)
L3_BYTES = 256 << 20    # Infinity Cache (MI355X_MICROARCH.md, Infinity Cache)
EVENT_EVERY = 4         # steps per sampled kernel timing inside the timed region
PARITY_STEPS = 64       # steps of the parity leg


def step_bytes(N, W, F):
    """Algorithmic HBM bytes per env-step: read the surviving window
    N(W-1)F*4 + the new bar N(F-1)*4 + the action N*4, write the next window NWF*4,
    value f64 read+write 16, reward 4  =  8*N*W*F + 20."""
    return 8 * N * W * F + 20


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg: the other window mode (--alt-steps), "
                         "the parity check against the CPU restatement (--parity-envs), the CPU baseline "
                         "(--cpu-baseline), the replay of the reference's recorded outputs, the non-finite count, "
                         "and at N > 1 the collective and --alt-weak-steps; off: their keys are null")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step handed its caller as DIR/<name>.npy: reward (f32, every "
                         "env), value (f64, every env) and obs (f32, the latest window of a fixed seeded sample "
                         "of envs, listed in obs_envs); ranks above 0 write <name>_rank<r>.npy")
    ap.add_argument("--global-envs", type=int, default=None,
                    help="strong scaling (the default): this many envs in total, sharded over the ranks "
                         "(north star / BASELINE config 4: 65,536 over 1/2/4/8 GPUs); default 65536")
    ap.add_argument("--envs-per-gpu", type=int, default=None,
                    help="weak scaling: this many envs per rank (implies --weak)")
    ap.add_argument("--weak", action="store_true",
                    help="weak scaling: --envs-per-gpu (default 65536) envs per rank instead of a fixed total")
    ap.add_argument("--alt-weak-steps", type=int, default=0,
                    help="N > 1, strong run: also time this many steps of the weak-scaled workload "
                         "(65,536 envs per rank), reported under alt_weak (0: skip)")
    ap.add_argument("--assets", type=int, default=30)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--features", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=256, help="resident days of synthetic bars/actions (cycled)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--cpu-baseline", type=int, default=1)
    ap.add_argument("--cpu-sample-envs", type=int, default=65536)
    ap.add_argument("--cpu-budget-s", type=float, default=20.0, help="target CPU-seconds of oracle work")
    ap.add_argument("--parity-envs", type=int, default=4096, help="envs of the parity leg checked on the CPU")
    ap.add_argument("--pmc-file", default=os.path.join(ROOT, "profiles", "pmc_traffic.json"))
    ap.add_argument("--windows", choices=["double", "inplace"], default="inplace")
    ap.add_argument("--reward", default="log_returns",
                    choices=["log_returns", "returns", "sharpe_ratio", "diff_sharpe"])
    ap.add_argument("--commission", type=float, default=0.0)
    ap.add_argument("--event-every", type=int, default=0,
                    help="timed steps per HIP-event-bracketed kernel sample; 0 (default): every 4th step, every "
                         "16th for Infinity-Cache-resident windows, whose steps take tens of us (an event pair costs "
                         "the stream ~1.5 us: 3.5 %% of a 4,096-env step sampled every 4th step)")
    ap.add_argument("--alt-steps", type=int, default=50,
                    help="extra timed steps of the other window mode (0: skip)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI; gloo lets several ranks share one GPU (functional rehearsal)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if not args.full:                                # the other legs' own options are read under --full only
        args.alt_steps = args.alt_weak_steps = args.cpu_baseline = 0
    if args.envs_per_gpu is not None or args.weak:
        if args.global_envs is not None:
            ap.error("--global-envs (strong scaling) and --envs-per-gpu / --weak (weak scaling) exclude each other")
        args.weak = True
        args.envs_per_gpu = args.envs_per_gpu or 65536
    elif args.global_envs is None:
        args.global_envs = 65536
    return args


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def host_cpus():
    """CPUs this process may use and the share the harness grants it (OMP_NUM_THREADS
    on the GPU box: one GPU's slice of the node)."""
    affinity = len(os.sched_getaffinity(0))
    share = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    return affinity, (min(share, affinity) if share > 0 else affinity)


def cpu_baseline(args, series, actions, H, torch):
    """The CPU restatement (oracle/pmenv_oracle.c, OpenMP over envs; test infrastructure
    used here as the timed baseline only) stepping the SAME workload shape — the full
    per-GPU env count, the same synthetic bars and actions — on the host cores, in place."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    from oracle import OracleEnv
    from pmenv import synth
    from pmenv.config import EnvConfig

    N, W, F = args.assets, args.window, args.features
    B = series.shape[1]
    S = min(args.cpu_sample_envs, B)
    Hc = min(16, H)                                            # distinct days cycled (host memory)
    obs = synth.window_from_series(series[:W, :S].contiguous(), W, F).cpu().numpy()
    bars = series[W:W + Hc, :S].cpu().numpy()
    acts = actions[:Hc, :S].cpu().numpy()
    affinity, threads = host_cpus()

    def run(envs, nthreads, budget_cpu_s):
        env = OracleEnv(EnvConfig(num_envs=envs, num_assets=N, window=W, features=F, reward=args.reward,
                                  commission=args.commission))
        o = np.ascontiguousarray(obs[:envs])
        b = [np.ascontiguousarray(bars[t, :envs]) for t in range(Hc)]
        a = [np.ascontiguousarray(acts[t, :envs]) for t in range(Hc)]
        env.reset(o)
        env.step(a[0], o, bar=b[0], threads=nthreads)          # first touch of the state
        steps, t0 = 0, time.perf_counter()
        while True:
            env.step(a[steps % Hc], o, bar=b[steps % Hc], threads=nthreads)
            steps += 1
            el = time.perf_counter() - t0
            if el * nthreads >= budget_cpu_s or steps >= 100000:
                return envs * steps / el, steps, el

    rate, steps, el = run(S, threads, args.cpu_budget_s)
    s1 = min(S, 4096)
    rate1, steps1, el1 = run(s1, 1, min(5.0, args.cpu_budget_s / 4))
    return {
        "value": rate, "unit": "env-steps/s", "cores": threads, "kind": "port",
        "sample": f"{S} envs x {steps} steps of the same N={N} W={W} F={F} fused in-place step "
                  f"(oracle/pmenv_oracle.c, OpenMP over envs, the bench's own synthetic bars and actions) "
                  f"in {el:.2f} s wall on {threads} threads (~{el * threads:.0f} CPU-s) of {cpu_model()}",
        "host_cpus": {"affinity": affinity, "nproc": os.cpu_count(), "threads_used": threads,
                      "note": "threads = the box's CPU share for one GPU (OMP_NUM_THREADS set by the "
                              "harness) when set, else every CPU in the affinity mask"},
        "single_thread": {"value": rate1, "sample": f"{s1} envs x {steps1} steps in {el1:.2f} s on 1 thread"},
    }


def parity_check(args, rec, lo, torch):
    """The parity leg's recorded GPU outputs vs the CPU restatement on the same inputs."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    from oracle import OracleEnv
    from pmenv.config import EnvConfig

    obs, bars, acts, g_r, g_v, g_obs = rec
    S = obs.shape[0]
    N, W, F = args.assets, args.window, args.features
    env = OracleEnv(EnvConfig(num_envs=S, num_assets=N, window=W, features=F, reward=args.reward,
                              commission=args.commission))
    env.reset(obs)
    _, threads = host_cpus()
    c_r = np.stack([env.step(acts[t], obs, bar=bars[t], threads=threads)[0] for t in range(acts.shape[0])])
    g_r = g_r.astype(np.float64)
    both_nan = np.isnan(g_r) & np.isnan(c_r)
    err = np.where(both_nan, 0.0, np.abs(g_r - c_r))
    return {"reward_mae": float(err.mean()),
            "reward_max_rel": float(np.max(np.where(both_nan, 0.0, err / (np.abs(c_r) + 1e-9)))),
            "value_max_rel": float(np.max(np.abs(g_v / env.value - 1.0))),
            "obs_bit_exact": bool(np.array_equal(g_obs, obs)),
            "sample": f"global envs {lo}..{lo + S - 1} of the timed handle x {acts.shape[0]} steps, "
                      f"HIP vs CPU restatement"}


def reference_golden_mae(dev, torch, TradingEnv):
    """Reward MAE / value error of the HIP path against the REFERENCE's own recorded
    outputs: tests/golden/simplex_n30_w50_t256_{f32,f64}.npz were written by running
    zachramsey/pm-rl's env/sim/trading_env.py (tests/golden/gen_golden.py) on a
    256-day, 30-asset, 50-day-window case; here one env replays the same windows and
    actions through the fused advance step (rank 0, after the timed region)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import golden_util as gu
    out = {}
    for name in ("simplex_n30_w50_t256_f32", "simplex_n30_w50_t256_f64"):
        g = gu.load(name)
        m = g["meta"]
        N, W, F, T = m["N"], m["W"], m["F"], m["T"]
        env = TradingEnv(num_envs=1, num_assets=N, window=W, features=F, device=dev)
        obs = None
        r = np.full(T + 1, np.nan)
        v = np.zeros(T + 1)
        for i in range(T + 1):
            if g["ops"][i]:
                obs = torch.as_tensor(gu.window(g, i)[0], dtype=torch.float32, device=dev).contiguous()
                env.reset(obs)
            else:
                ri, _ = env.step(torch.as_tensor(g["actions"][i], dtype=torch.float32, device=dev).reshape(N, 1),
                                 obs, bar=torch.as_tensor(gu.bar(g, i), dtype=torch.float32, device=dev))
                r[i] = float(ri)
            v[i] = float(env.value)
        ok = ~g["ops"].astype(bool) & np.isfinite(g["rewards"])
        out[m["dtype"]] = {"reward_mae": float(np.mean(np.abs(r[ok] - g["rewards"][ok]))),
                           "value_max_rel": float(np.max(np.abs(v / g["values"] - 1.0))), "steps": int(ok.sum())}
    return {"case": "simplex_n30_w50_t256 (reference env outputs recorded in tests/golden)", **out}


def weak_leg(args, rank, world, dev, lib, _abi, synth, TradingEnv, torch, dist):
    """The weak-scaled workload beside a strong-scaled run: 65,536 envs per rank (global ids
    rank * 65,536 ..), in place, `--alt-weak-steps` steps between barriers, max over ranks."""
    N, W, F, B = args.assets, args.window, args.features, 65536
    steps = args.alt_weak_steps
    H = max(1, min(args.horizon, steps + 4))
    series = synth.series(H + W, B, N, env_offset=rank * B, seed=args.seed, device=dev)
    actions = synth.actions(H, B, N, env_offset=rank * B, seed=args.seed + 1, device=dev)
    obs = synth.window_from_series(series, W, F)
    env = TradingEnv(num_envs=B, num_assets=N, window=W, features=F, device=dev,
                     reward=args.reward, commission=args.commission)
    env.reset(obs)
    reward = torch.empty(B, dtype=torch.float32, device=dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    blocks = []
    for t in range(H):
        a = _abi.PmenvStepArgs()
        a.action, a.bar, a.obs, a.reward = actions[t].data_ptr(), series[W + t].data_ptr(), obs.data_ptr(), \
            reward.data_ptr()
        blocks.append((a, ctypes.byref(a)))
    for i in range(4):
        _abi.check(lib.pmenv_step_ex(env._h, blocks[i % H][1], sp), env._h, "pmenv_step_ex")
    torch.cuda.synchronize(dev)
    dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(steps):
        _abi.check(lib.pmenv_step_ex(env._h, blocks[(4 + i) % H][1], sp), env._h, "pmenv_step_ex")
    torch.cuda.synchronize(dev)
    dist.barrier()
    torch.cuda.synchronize(dev)
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64,
                      device=dev if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(el, op=dist.ReduceOp.MAX)
    el = float(el[0])
    out = {"scaling": "weak", "envs_per_gpu": B, "global_envs": world * B, "steps": steps,
           "value": world * B * steps / el, "unit": "env-steps/s", "ms_per_step": el / steps * 1e3,
           "step_path": env.step_path.split(" | ")[-1], "nonfinite_envs": env.nonfinite_count()}
    env.close()
    return out


def lib_source_sha256():
    """sha256 of the product library's sources and build script (tools/libfp.py), or None."""
    try:
        from tools.libfp import source_sha256
    except ImportError:
        return None
    return source_sha256(ROOT)


def sha256_file(path):
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


DUMP_BYTES = 40 * 10**6   # --dump-outputs: budget of the sampled window
DUMP_TOTAL = 60 * 10**6   # ... and of the whole dump


def dump_outputs(args, rank, reward, value, window):
    """--dump-outputs: what the last timed step handed its caller, as DIR/<name>.npy — the
    reward (f32 [B]) and the portfolio value (f64 [B]) of every env, and the latest window
    (f32 [n, N, W, F]) of a fixed sample of envs drawn from --seed (every env when they fit
    DUMP_BYTES); obs_envs lists the sampled env ids (f64). Past a million envs the reward and
    the value are the sample's as well. The inputs are a function of the arguments alone, so
    two builds run with the same arguments are compared file by file."""
    import numpy as np
    import torch
    B = reward.shape[0]
    n = max(1, min(B, DUMP_BYTES // (window[0].numel() * 4)))
    ids = np.sort(np.random.default_rng(args.seed).choice(B, size=n, replace=False)) if n < B else np.arange(B)
    sel = torch.as_tensor(ids, device=window.device)
    out = {"reward": reward, "value": value, "obs": window.index_select(0, sel), "obs_envs": ids}
    if B * 12 > DUMP_TOTAL - DUMP_BYTES - ids.size * 8:
        out["reward"], out["value"] = reward.index_select(0, sel), value.index_select(0, sel)
    os.makedirs(args.dump_outputs, exist_ok=True)
    sfx = f"_rank{rank}" if rank else ""
    for name, a in out.items():
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        np.save(os.path.join(args.dump_outputs, f"{name}{sfx}.npy"),
                np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64))


def spread(us):
    """min / median / max of the sampled kernel times, and which sample was the slowest
    (sample i brackets timed step EVENT_EVERY * i, or 4 EVENT_EVERY * i for cache-resident windows)."""
    return {"min": min(us), "median": statistics.median(us), "max": max(us), "samples": len(us),
            "slowest_sample": max(range(len(us)), key=us.__getitem__)}


def main():
    args = parse()
    knobs = {k: v for k, v in os.environ.items() if k.startswith("PMENV_")}
    if knobs:
        sys.exit(f"bench.py refuses to time with PMENV_* variables set: {sorted(knobs)} "
                 "(the product library reads none; A/B variants live in the tools build)")
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one process per GPU)")
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local % max(ndev, 1))
    torch.cuda.set_device(dev)
    if world > 1:
        # RCCL ("nccl") over xGMI; --dist-backend gloo lets several ranks share one GPU for
        # functional rehearsal (RCCL refuses two ranks on one device)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    from pmenv import TradingEnv, synth, _abi
    lib = _abi.load()

    N, W, F = args.assets, args.window, args.features
    if not args.weak:                                # strong scaling: a shard of a fixed total
        from pmenv.parallel import shard_range
        lo, hi = shard_range(args.global_envs, rank, world)
        B = hi - lo
        args.envs_per_gpu = B
    else:                                            # weak scaling: global env ids of this rank
        B = args.envs_per_gpu
        lo = rank * B
    H = max(1, min(args.horizon, max(PARITY_STEPS, args.steps + args.warmup)))
    series = synth.series(H + W, B, N, env_offset=lo, seed=args.seed, device=dev)      # [H+W, B, N, 4]
    actions = synth.actions(H, B, N, env_offset=lo, seed=args.seed + 1, device=dev)     # [H, B, N]
    obs = synth.window_from_series(series, W, F)                                         # [B, N, W, F]
    env = TradingEnv(num_envs=B, num_assets=N, window=W, features=F, device=dev,
                     reward=args.reward, commission=args.commission)
    obs_b = torch.empty_like(obs) if (args.windows == "double" or args.alt_steps > 0) else None
    reward = torch.empty(B, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    h = env._h
    bar_ptrs = [series[W + t].data_ptr() for t in range(H)]
    act_ptrs = [actions[t].data_ptr() for t in range(H)]
    step_fn = lib.pmenv_step_ex
    ping_ptr = [obs.data_ptr(), obs_b.data_ptr() if obs_b is not None else None]
    paths = env.step_path.split(" | ")              # "<double-buffered> (obs_out) | <in place> (in place)"
    # one prebuilt argument block per (day, window mode, ping-pong side, phase): the host
    # work per step is then one ctypes call (small configs are otherwise host-bound)
    arg_cache = {}

    def step_args(t, double, side, phases):
        key = (t, double, side, phases)
        hit = arg_cache.get(key)
        if hit is None:
            a = _abi.PmenvStepArgs()
            a.reward = reward.data_ptr()
            a.action, a.bar = act_ptrs[t], bar_ptrs[t]
            a.obs = ping_ptr[side] if double else ping_ptr[0]
            a.obs_out = ping_ptr[1 - side] if double else None
            a.phases = phases
            hit = arg_cache[key] = (a, ctypes.byref(a))
        return hit[1]

    def one_step(i, double, phase_events=None):
        phased = "+" in paths[0 if double else -1]  # two launches: time the window stream on its own
        t = i % H
        side = i % 2
        if phase_events is None:
            rc = step_fn(h, step_args(t, double, side, 0), sp)
        elif phased:
            # same two launches as phases=0, with an event between them so the
            # streaming kernel is timed on its own stream
            rc = step_fn(h, step_args(t, double, side, _abi.PHASE_SCALAR), sp)
            phase_events[0].record(stream)
            rc = rc or step_fn(h, step_args(t, double, side, _abi.PHASE_ADVANCE), sp)
            phase_events[1].record(stream)
        else:                                        # one launch per step: time that launch
            phase_events[0].record(stream)
            rc = step_fn(h, step_args(t, double, side, 0), sp)
            phase_events[1].record(stream)
        if rc != 0:
            _abi.check(rc, h, "pmenv_step_ex")

    # ---- 1. lead-in on the timed handle (every rank): the steps that bring the clocks up.
    # Under --full they are the parity leg as well; its records stay on the GPU until after
    # the timed region: no host copy (and no idle GPU) between this leg and the timed
    # steps, so the clocks it brought up are still up when the timing starts.
    S = min(args.parity_envs if world == 1 else 256, B)
    if args.full:
        rec_obs0 = obs[:S].clone()
    env.reset(obs)
    if args.full:
        rec_r = torch.empty(PARITY_STEPS, S, dtype=torch.float32, device=dev)
    for i in range(PARITY_STEPS):
        one_step(i, False)
        if args.full:
            rec_r[i].copy_(reward[:S])
    if args.full:
        rec_v, rec_obs = env.value[:S].clone(), obs[:S].clone()
    # back to the initial window and a fresh env state for the timed legs
    obs.copy_(synth.window_from_series(series, W, F))
    env.reset(obs)

    # ---- 2. the timed region
    def timed(steps, warmup, double):
        for i in range(warmup):
            one_step(i, double)
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)
        # the stream kernel (or the one-launch step) is bracketed by HIP events on every
        # EVENT_EVERY-th step of the timed region (each event pair costs the stream a few us)
        # the same on every rank: a function of the shape, not of a measurement
        every = args.event_every if args.event_every > 0 else (
            EVENT_EVERY if B * N * W * F * 4 * (2 if double else 1) > L3_BYTES else 4 * EVENT_EVERY)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(0, steps, every)]
        t0 = time.perf_counter()
        for i in range(steps):
            one_step(warmup + i, double, ev[i // every] if i % every == 0 else None)
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        timed.every = every
        return el, [a.elapsed_time(b) * 1e3 for a, b in ev]

    double = args.windows == "double"
    elapsed, k_us = timed(args.steps, args.warmup, double)
    ev_every = timed.every
    kern_avg_s = sum(k_us) / len(k_us) / 1e6
    if args.dump_outputs:
        # the last timed step's window: in place it is obs; double-buffered, the side it wrote
        last = args.warmup + args.steps - 1
        dump_outputs(args, rank, reward, env.value, obs_b if double and last % 2 == 0 else obs)
    alt = None
    if args.alt_steps > 0:
        # the other window mode, continuing from the latest window
        if double and (args.warmup + args.steps) % 2:
            obs.copy_(obs_b)
        a_el, a_k = timed(args.alt_steps, 2, not double)
        alt = {"windows": "inplace" if double else "double",
               "env_steps_per_s_per_gpu": B * args.alt_steps / a_el,
               "ms_per_step": a_el / args.alt_steps * 1e3, "kernel_avg_us": sum(a_k) / len(a_k),
               "kernel_us": spread(a_k)}

    collective = None
    if world > 1:
        t = torch.tensor([elapsed, kern_avg_s], dtype=torch.float64,
                         device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, kern_avg_s = float(t[0]), float(t[1])
    if world > 1 and args.full:
        # the path's one exchange (outside the timed step loop): the advantage-
        # normalisation moments of the last rewards, {count, sum, sum of squares} f64
        # from the HIP moments kernel, summed over ranks (pmenv.parallel.normalize)
        from pmenv import parallel
        adv = reward                                              # device tensor (gloo stages it)
        parallel.normalize(adv)                                   # warm
        torch.cuda.synchronize(dev)
        dist.barrier()
        c0 = time.perf_counter()
        reps = 20
        for _ in range(reps):
            normed = parallel.normalize(adv)
        torch.cuda.synchronize(dev)
        c_us = (time.perf_counter() - c0) / reps * 1e6
        n_all, _, _ = parallel.allreduce_moments(parallel.local_moments_cpu(adv).to(adv.device))
        collective = {"op": "all_reduce(sum) of 24-byte advantage moments + normalise", "backend": dist.get_backend(),
                      "us_per_update": c_us, "count_all_ranks": n_all, "normalised_finite": bool(torch.isfinite(normed).all())}
    alt_weak = None
    if world > 1 and not args.weak and args.alt_weak_steps > 0:
        alt_weak = weak_leg(args, rank, world, dev, lib, _abi, synth, TradingEnv, torch, dist)

    # ---- 4. checks and baselines (--full, after the timed region)
    nonfinite = parity = cpu = ref_gold = None
    if args.full:
        nonfinite = env.nonfinite_count()
        idx = [t % H for t in range(PARITY_STEPS)]      # the leg cycles through the H resident days
        rec = (rec_obs0.cpu().numpy(), series[W:W + H, :S].cpu().numpy()[idx],
               actions[:, :S].cpu().numpy()[idx], rec_r.cpu().numpy(), rec_v.cpu().numpy(), rec_obs.cpu().numpy())
        del rec_obs0, rec_obs
        parity = parity_check(args, rec, lo, torch)
        if world > 1:
            t = torch.tensor([parity["reward_max_rel"], parity["value_max_rel"],
                              0.0 if parity["obs_bit_exact"] else 1.0],
                             dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            parity.update({"reward_max_rel_all_ranks": float(t[0]), "value_max_rel_all_ranks": float(t[1]),
                           "obs_bit_exact_all_ranks": float(t[2]) == 0.0})
        if rank == 0 and world == 1 and args.cpu_baseline:
            cpu = cpu_baseline(args, series, actions, H, torch)
            ref_gold = reference_golden_mae(dev, torch, TradingEnv)

    kernel = paths[0 if double else -1].split(" (")[0].split("+")[-1]
    total_env_steps = (world * B if args.weak else args.global_envs) * args.steps
    value = total_env_steps / elapsed
    bstep = step_bytes(N, W, F)
    achieved_event = bstep * B / kern_avg_s / 1e9
    achieved_step = bstep * B / (elapsed / args.steps) / 1e9
    # which kernel time the headline frac divides by: the HIP-event mean of the dominant kernel
    # (bracketed on every ev_every-th step), unless that mean exceeds the unbracketed wall-clock
    # ms_per_step — then the event pair itself is inflating it and the step time is the honest one
    if kern_avg_s > elapsed / args.steps:
        achieved, frac_source = achieved_step, (
            "ms_per_step (unbracketed wall-clock of the timed region / steps): the HIP-event mean "
            "exceeds it, so the event pair inflates the bracketed launch")
    else:
        achieved, frac_source = achieved_event, (
            f"kernel_avg_us (HIP events on the launch stream around the dominant kernel, "
            f"every {ev_every}th timed step)")
    window_bytes = B * N * W * F * 4
    traffic, traffic_src = None, None
    lib_sha = sha256_file(_abi.LIB_PATH)
    src_sha = lib_source_sha256()
    try:
        pmc = json.load(open(args.pmc_file))
        # rocprofv3 FETCH_SIZE / WRITE_SIZE passes (tools/pmc_summary.py) of the same kernel at
        # the same workload, measured on THIS library — the same binary, or (hipcc output is
        # not byte-reproducible) a build of the same sources and build script: anything else
        # reports null rather than a stale figure
        same = pmc.get("workload") == [B, N, W, F] and f"::{kernel}<" in pmc.get("dominant_kernel", "")
        same_bin = pmc.get("lib_sha256") == lib_sha
        same_src = src_sha is not None and pmc.get("lib_src_sha256") == src_sha
        traffic_src = {"file": os.path.relpath(args.pmc_file, ROOT), "tag": pmc.get("tag"),
                       "lib_sha256": pmc.get("lib_sha256"), "running_lib_sha256": lib_sha,
                       "lib_src_sha256": pmc.get("lib_src_sha256"), "running_lib_src_sha256": src_sha,
                       "same_workload_and_kernel": same, "same_binary": same_bin, "same_sources": same_src,
                       "same_library": same_bin or same_src}
        if same and traffic_src["same_library"]:
            traffic = pmc.get("hbm_bytes_per_launch")
    except (OSError, ValueError):
        pass

    l3 = window_bytes * (2 if double else 1) <= L3_BYTES
    if rank == 0:
        line = {
            "metric": "env-steps/sec (whole node) at 65k envs x 30 assets; reward MAE vs CPU ref",
            "value": value,
            "unit": "env-steps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak" if args.weak else "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (Philox OHLC random walk + softmax actions, resident in HBM)",
            "config": {
                "workload": (f"fused env step, {world * B if args.weak else args.global_envs} envs in total "
                             f"({B} envs/GPU) x {N} assets x {W}-day window x {F} channels"),
                "envs_per_gpu": B, "global_envs": world * B if args.weak else args.global_envs,
                "assets": N, "window": W, "features": F,
                "reward": args.reward, "commission": args.commission, "obs_dtype": "f32", "accumulate": "f64",
                "windows": args.windows,
                "parallelism": f"env-sharded x{world} (no collective in the step)",
                # what one rank's share runs as (rank 0): at N = 8 the 65,536-env job is 8,192
                # envs per GPU, an Infinity-Cache-resident window on its own step path
                "per_rank": {"envs": B, "window_bytes": window_bytes, "l3_resident": l3,
                             "step_path": paths[0 if double else -1]},
            },
            "roofline": {
                "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS, "frac_source": frac_source,
                "traffic": traffic, "traffic_source": traffic_src,
                "kernel": kernel, "kernel_avg_us": kern_avg_s * 1e6, "kernel_us": spread(k_us),
                "achieved_event": achieved_event, "frac_event": achieved_event / HBM_PEAK_GBS,
                "bytes_per_env_step": bstep,
                "achieved_step": achieved_step, "frac_step": achieved_step / HBM_PEAK_GBS,
                "l3_resident": l3,
                "note": ("the window (x2 double-buffered) fits the 256 MiB Infinity Cache: frac is not an HBM fraction"
                         if l3 else "window streams through HBM (larger than the 256 MiB Infinity Cache)"),
            },
            "cpu_baseline": cpu,
            "full": args.full,
            "reward_mae": parity and parity["reward_mae"],
            "parity_sample": parity,
            "reference_goldens": ref_gold,
            "nonfinite_envs": nonfinite,
            "step_path": env.step_path,
            # the library this line measured (the configs summaries print it: tools/bench_configs.sh)
            "library": {"path": os.path.relpath(_abi.LIB_PATH, ROOT), "sha256": lib_sha, "src_sha256": src_sha},
            "knobs": knobs,
            "alt": alt,
            "collective": collective,
            "alt_weak": alt_weak,
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
