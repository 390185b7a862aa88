"""One train/off_policy.py epoch (collect -> update sampling) at BASELINE config 3
(16,384 envs x 30 assets, off-policy + replay/buffer.py on device, 1 GPU) over
pmenv.off_policy.OffPolicy: every env trades one HBM-resident series, each step is
recorded in the device replay, and the update phase samples (s, a, r, s') batches
through the HIP gather.

The agent (DSAC / TD3) is out of scope: `act` is a random simplex and `update` a
no-op, so the times below are the env, data and replay side of an epoch only.
Prints one JSON object; `--out` writes it too.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pm-rl_amd"))
import torch  # noqa: E402

from pmenv import MarketSeries, TradingEnv, synth  # noqa: E402
from pmenv.off_policy import OffPolicy  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=16384)
ap.add_argument("--assets", type=int, default=30)
ap.add_argument("--window", type=int, default=50)
ap.add_argument("--days", type=int, default=1024, help="resident series length")
ap.add_argument("--steps", type=int, default=64, help="collect steps per epoch")
ap.add_argument("--capacity", type=int, default=128)
ap.add_argument("--updates", type=int, default=64)
ap.add_argument("--batch-size", type=int, default=1024)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--prioritized", action="store_true",
                help="draw by priority (the sum tree is kept current by add) and feed |r| back as the TD error")
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
B, N, W = a.envs, a.assets, a.window
m = MarketSeries(synth.series(a.days, 1, N, device=dev)[:, 0].contiguous(), device=dev)
env = TradingEnv(num_envs=B, num_assets=N, window=W, device=dev)
ap_gen = torch.Generator(device=dev).manual_seed(1)     # sample indices drawn on the GPU
if a.prioritized:
    loop = OffPolicy(env, m, capacity=a.capacity, update=lambda s, a_, r, s2, w: r.reshape(-1),
                     batch_size=a.batch_size, generator=ap_gen, prioritized=True)
else:
    loop = OffPolicy(env, m, capacity=a.capacity, update=lambda *x: None, batch_size=a.batch_size, generator=ap_gen)
gen = torch.Generator().manual_seed(2)
st = torch.cuda.current_stream()
E = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

step_ev = []
_step = env.step


def timed_step(*args, **kw):
    e0, e1 = E(), E()
    e0.record(st)
    out = _step(*args, **kw)
    e1.record(st)
    step_ev.append((e0, e1))
    return out


env.step = timed_step
res = []
for it in range(a.iters + 1):
    step_ev.clear()
    start = m.random_starts(B, W, a.steps, generator=gen)
    t0, t1, t2 = E(), E(), E()
    t0.record(st)
    loop.collect(start, a.steps, random=True)
    t1.record(st)
    loop.update(a.updates)
    t2.record(st)
    torch.cuda.synchronize()
    if it == 0:
        continue
    env_ms = sum(x.elapsed_time(y) for x, y in step_ev)
    col = t0.elapsed_time(t1)
    res.append({"collect_ms": col, "env_step_ms": env_ms, "action_and_replay_add_ms": col - env_ms,
                "update_sampling_ms": t1.elapsed_time(t2)})
med = {k: sorted(r[k] for r in res)[len(res) // 2] for k in res[0]}
S = a.updates * a.batch_size
doc = {"device": torch.cuda.get_device_name(0), "envs": B, "assets": N, "window": W, "collect_steps": a.steps,
       "capacity": a.capacity, "prioritized": a.prioritized, "updates": a.updates, "batch_size": a.batch_size, "median": med,
       "env_steps_per_s_collect": B * a.steps / (med["collect_ms"] / 1e3),
       "env_steps_per_s_env_only": B * a.steps / (med["env_step_ms"] / 1e3),
       "samples_per_s": S / (med["update_sampling_ms"] / 1e3),
       "sample_write_GBs": S * (2 * N * W * 5 * 4 + N * 4 + 4) / (med["update_sampling_ms"] / 1e3) / 1e9,
       "note": "act = random simplex, update = no-op (agent out of scope); env in resident-series mode"}
print(json.dumps(doc, indent=1))
if a.out:
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
