"""The per-env replay's device paths on an MI355X at config 3's ring (16,384 envs x 256 rows,
N 30, W 50, episodes of 64-200 rows per env) -> profiles/rows_replay_env.json.

(a) pmenv_replay_valid_build (need = W + 1, W + 64) and pmenv_replay_valid_select (S = 256,
    8,192) against the torch composition a user would otherwise write: ep[rows] == ep[rows +
    need - 1] -> nonzero -> randint index.
(b) the per-env n-step (n = 5, 64) and sequence (16 x 64, 128 x 64) gathers against the
    lockstep gathers on the same ring and indices: `same` feeds the per-env entry point an
    [H, B] array whose columns all repeat the lockstep [H] ids (the same fold lengths: the
    difference is the id addressing alone), `own` the ring's own per-env ids.
(c) with --parent-lib: the lockstep gathers of this build against another build's library
    (the parent commit's), both loaded into this process.

Every pair is timed in one process, alternating, five rounds of bench_rows.timeit's medians
(the method of rows_prio.json); `spread` is (max - min) / median over a side's rounds.

    python tools/bench_replay_env.py --out profiles/rows_replay_env.json [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pm-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench_rows import P, timeit  # noqa: E402
from pmenv import _abi  # noqa: E402


def bind(path):
    lib = ctypes.CDLL(path)
    for name, res, args in _abi.SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--assets", type=int, default=30)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--commit", default=None, help="the commit the parent library was built from (recorded)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _abi.load()
    B, H, N, W, F = a.envs, a.rows, a.assets, a.window, 5
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(11)
    rng = np.random.default_rng(11)

    def ck(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    # a full ring (count == H, oldest mid-array): env b's episodes take 64 .. 200 rows each
    T = H + W + 8
    series = torch.randn(T, N, F - 1, device=dev, generator=g)
    days = (torch.arange(H, dtype=torch.int32, device=dev)[:, None] + W).expand(H, B).contiguous()
    actions = torch.rand(H, B, N, device=dev, generator=g)
    rewards = torch.randn(H, B, device=dev, generator=g)
    oldest, count = 77, H
    done = np.zeros((H, B), dtype=bool)
    nxt = rng.integers(0, 200, B)
    for t in range(H):
        hit = nxt == t
        done[t] = hit
        nxt[hit] += rng.integers(64, 201, int(hit.sum()))
    chrono = np.concatenate([np.zeros((1, B), np.int32), done[:-1].cumsum(0).astype(np.int32)])
    ep = torch.as_tensor(np.roll(chrono, oldest, axis=0), device=dev).contiguous()       # [H, B]
    ep_row = ep[:, 0].contiguous()                                                        # the lockstep ids [H]
    ep_same = ep_row[:, None].expand(H, B).contiguous()
    # lockstep rows take the days of a ring written in row order from `oldest`
    days = torch.roll(days, oldest, 0).contiguous()
    res = []

    def pair(name, hip, ref, ref_name, **kw):
        """Five alternating rounds; both sides' medians and spreads, and whether the
        difference lies inside the larger spread."""
        hip()
        ref()
        th, tr = [], []
        for _ in range(5):
            th.append(timeit(hip, a.reps))
            tr.append(timeit(ref, a.reps))
        us, base = statistics.median(th), statistics.median(tr)
        sp_h, sp_r = (max(th) - min(th)) / us, (max(tr) - min(tr)) / base
        d = {"case": name, "us": round(us, 2), "spread": round(sp_h, 4), "baseline": ref_name,
             "baseline_us": round(base, 2), "baseline_spread": round(sp_r, 4), "ratio": round(us / base, 4),
             "inside_spread": bool(abs(us - base) <= max(sp_h * us, sp_r * base))}
        d.update(kw)
        print(json.dumps(d), file=sys.stderr)
        res.append(d)

    # ---- (a) the map and the draw
    WB = (B + 63) // 64
    maps = {}
    for need in (W + 1, W + 64):
        span = count - need
        bits = torch.empty(span, WB, dtype=torch.int64, device=dev)
        rowsum = torch.empty(span + 1, dtype=torch.int64, device=dev)
        got = {}

        def build():
            ck(lib.pmenv_replay_valid_build(P(ep), H, B, oldest, count, need, P(bits), P(rowsum), st), "valid_build")

        def build_torch():
            rows = (oldest + torch.arange(span, device=dev)) % H
            got["idx"] = (ep[rows] == ep[(rows + need - 1) % H]).nonzero()
        pair(f"valid_build_need{need}", build, build_torch, "torch: ep[rows] == ep[rows + need - 1] -> nonzero",
             need=need, span=span, B=B, alg_bytes=2 * span * B * 4 + span * WB * 8)
        total = int(rowsum[-1])
        assert total == got["idx"].shape[0], (total, got["idx"].shape)
        res[-1]["total"] = total
        maps[need] = (bits, rowsum, got["idx"], total)
    bits, rowsum, idx, total = maps[W + 1]
    span = count - W - 1
    for S in (256, 8192):
        u = torch.rand(S, dtype=torch.float64, device=dev, generator=g)
        h0 = torch.empty(S, dtype=torch.int32, device=dev)
        env = torch.empty(S, dtype=torch.int32, device=dev)
        got = {}

        def select():
            ck(lib.pmenv_replay_valid_select(P(bits), P(rowsum), H, B, oldest, span, P(u), S, P(h0), P(env), st),
               "valid_select")

        def select_torch():
            p = idx[torch.randint(0, total, (S,), device=dev)]
            got["h0"], got["env"] = ((oldest + p[:, 0]) % H).to(torch.int32), p[:, 1].to(torch.int32)
        pair(f"valid_select_S{S}", select, select_torch, "torch: randint index into the nonzero list", S=S, total=total)
        k = (u * total).floor().long().clamp_(0, total - 1)
        want = idx[k]
        res[-1]["exact"] = bool(torch.equal(env.long(), want[:, 1]) and torch.equal(h0.long(), (oldest + want[:, 0]) % H))

    # ---- (b), (c) the gathers
    def draw(ids, S):
        b_, r_ = torch.empty(span, WB, dtype=torch.int64, device=dev), torch.empty(span + 1, dtype=torch.int64, device=dev)
        ck(lib.pmenv_replay_valid_build(P(ids), H, B, oldest, count, W + 1, P(b_), P(r_), st), "valid_build")
        h0 = torch.empty(S, dtype=torch.int32, device=dev)
        env = torch.empty(S, dtype=torch.int32, device=dev)
        u = torch.rand(S, dtype=torch.float64, device=dev, generator=g)
        ck(lib.pmenv_replay_valid_select(P(b_), P(r_), H, B, oldest, span, P(u), S, P(h0), P(env), st), "valid_select")
        assert int(h0.min()) >= 0
        return h0, env

    def nstep_call(L, fn, ids, h0, env, S, n, out):
        s, s2, ao, ro, steps, disc = out
        return lambda: ck(getattr(L, fn)(P(series), T, N, F, W, P(days), P(actions), P(rewards), H, B, P(h0), P(env), S,
                                         P(ids), oldest, count, n, 0.997, P(s), P(s2), P(ao), P(ro), P(steps), P(disc),
                                         st), fn)

    def seq_call(L_, fn, ids, h0, env, S, L, out):
        x, ao, ro, ln = out
        return lambda: ck(getattr(L_, fn)(P(series), T, N, F, W, P(days), P(actions), P(rewards), H, B, P(h0), P(env), S,
                                          P(ids), oldest, count, L, 1, P(x), P(ao), P(ro), P(ln), st), fn)

    parent = bind(a.parent_lib) if a.parent_lib else None
    S = 8192
    h0s, envs = draw(ep_same, S)
    h0o, envo = draw(ep, S)
    out = (torch.empty(S, N, W, F, device=dev), torch.empty(S, N, W, F, device=dev), torch.empty(S, N, device=dev),
           torch.empty(S, device=dev), torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, device=dev))
    for n in (5, 64):
        lock = nstep_call(lib, "pmenv_replay_gather_nstep", ep_row, h0s, envs, S, n, out)
        same = nstep_call(lib, "pmenv_replay_gather_nstep_env", ep_same, h0s, envs, S, n, out)
        own = nstep_call(lib, "pmenv_replay_gather_nstep_env", ep, h0o, envo, S, n, out)
        lock()
        m_lock = out[4].clone()
        same()
        assert torch.equal(m_lock, out[4])
        pair(f"nstep_env_same_S{S}_n{n}", same, lock, "lockstep pmenv_replay_gather_nstep, same ring and indices", S=S, n=n)
        pair(f"nstep_env_own_S{S}_n{n}", own, lock, "lockstep pmenv_replay_gather_nstep, same ring", S=S, n=n)
        if parent is not None:
            old = nstep_call(parent, "pmenv_replay_gather_nstep", ep_row, h0s, envs, S, n, out)
            pair(f"nstep_lockstep_vs_parent_S{S}_n{n}", lock, old, "the parent build's pmenv_replay_gather_nstep", S=S,
                 n=n, parent=a.commit)
    del out
    for Sq, L in ((16, 64), (128, 64)):
        h0s, envs = draw(ep_same, Sq)
        h0o, envo = draw(ep, Sq)
        out = (torch.empty(L, Sq, N, W, F, device=dev), torch.empty(L, Sq, N, device=dev),
               torch.empty(L, Sq, device=dev), torch.empty(Sq, dtype=torch.int32, device=dev))
        lock = seq_call(lib, "pmenv_replay_gather_seq", ep_row, h0s, envs, Sq, L, out)
        same = seq_call(lib, "pmenv_replay_gather_seq_env", ep_same, h0s, envs, Sq, L, out)
        own = seq_call(lib, "pmenv_replay_gather_seq_env", ep, h0o, envo, Sq, L, out)
        lock()
        m_lock = out[3].clone()
        same()
        assert torch.equal(m_lock, out[3])
        pair(f"seq_env_same_S{Sq}_L{L}", same, lock, "lockstep pmenv_replay_gather_seq, same ring and indices", S=Sq, L=L)
        pair(f"seq_env_own_S{Sq}_L{L}", own, lock, "lockstep pmenv_replay_gather_seq, same ring", S=Sq, L=L)
        if parent is not None:
            old = seq_call(parent, "pmenv_replay_gather_seq", ep_row, h0s, envs, Sq, L, out)
            pair(f"seq_lockstep_vs_parent_S{Sq}_L{L}", lock, old, "the parent build's pmenv_replay_gather_seq", S=Sq,
                 L=L, parent=a.commit)
        del out

    doc = {"device": torch.cuda.get_device_name(0), "ring": {"B": B, "H": H, "N": N, "W": W, "episode_rows": "64-200"},
           "method": "one process, alternating, 5 rounds of medians over reps groups of 10 calls; spread = (max - min) / median",
           "parent": a.commit, "cases": res}
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
