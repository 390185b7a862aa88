"""Measure the SURVEY.md §8f kernels (f1 GAE + moments, f2 batched reward, f3
resident-series advance, f4 replay gather + metrics) against their algorithmic bytes.

Every case calls the C ABI directly on preallocated device buffers (what a training
loop does), timed with HIP events on torch's current stream — the stream the calls
enqueue on — per call, as the median over `--reps` groups of 10 back-to-back calls
after warmup. A case is one ABI call (its kernels and the boundaries between them,
no allocation). Run under
`rocprofv3 --kernel-trace --stats` for per-kernel durations.
Prints one JSON object; `--out` writes it too.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PMENV_LIB", os.path.join(ROOT, "tools", "libpmenv_ab.so"))  # the A/B knobs: tools build
sys.path.insert(0, os.path.join(ROOT, "pm-rl_amd"))
import torch  # noqa: E402

from pmenv import MarketSeries, TradingEnv, synth, _abi  # noqa: E402
from pmenv.replay import DeviceReplay  # noqa: E402

PEAK_GBS = 8000.0


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timeit(fn, reps, warmup=3, inner=10):
    """Median over `reps` groups of `inner` back-to-back calls (per call): launch
    latency overlaps the previous call, as in a training loop."""
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


def row(name, us, alg_bytes, **kw):
    gbs = alg_bytes / us / 1e3
    d = {"case": name, "us": round(us, 2), "alg_bytes": int(alg_bytes), "GBs": round(gbs, 1),
         "frac_8TBs": round(gbs / PEAK_GBS, 3)}
    d.update(kw)
    print(json.dumps(d), file=sys.stderr)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="comma list of f1,f2,f3,f4,prio,rollout_env (default: all; rollout_env is part of f1)")
    ap.add_argument("--parent-lib", default="", help="rollout_env: another build's libpmenv.so (the parent commit's), "
                    "whose pmenv_rollout_gather is timed beside this build's in the same process")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"f1", "f2", "f3", "f4", "prio"}
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _abi.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev).manual_seed(0)
    res = []

    def ck(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    if "f1" in only:
        # GAE over a time-major rollout: per-env loop, wave scan, tiled scan (U = 8, 16)
        for T, B, dn in ((256, 65536, True), (256, 16384, True), (256, 4096, True), (2048, 8192, True),
                         (4096, 512, True), (16384, 64, False)):
            r = torch.randn(T, B, device=dev, generator=g)
            v = torch.randn(T + 1, B, device=dev, generator=g)
            d = (torch.rand(T, B, device=dev, generator=g) < 0.01).to(torch.uint8) if dn else None
            adv, ret = torch.empty_like(r), torch.empty_like(r)
            alg = T * B * (4 + 4 + 4 + 4 + (1 if dn else 0)) + B * 4
            big = T * B <= (1 << 24)
            modes = {"loop": {"PMENV_GAE": "loop"}, "scan": {"PMENV_GAE": "scan"}} if big else {}
            modes.update({"tile": {"PMENV_GAE": "tile", "PMENV_GAE_U": "8"},
                          "tile16": {"PMENV_GAE": "tile", "PMENV_GAE_U": "16"},
                          "tile_occ8": {"PMENV_GAE": "tile8"},
                          "stream8": {"PMENV_GAE": "stream", "PMENV_GAE_P": "8"},
                          "stream16": {"PMENV_GAE": "stream", "PMENV_GAE_P": "16"},
                          "stream32": {"PMENV_GAE": "stream", "PMENV_GAE_P": "32"},
                          "tile_nt": {"PMENV_GAE_SP": "2"},
                          "tile_sc1": {"PMENV_GAE_SP": "16"},
                          "auto": {}})
            nbytes = lib.pmenv_gae_workspace(T, B)
            work = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
            gk = ("PMENV_GAE", "PMENV_GAE_U", "PMENV_GAE_P", "PMENV_GAE_SP")
            outs = {}
            for mode, env in modes.items():
                for k in gk:
                    os.environ.pop(k, None)
                os.environ.update(env)
                # auto = what rollout.gae runs: pmenv_gae_ex with its workspace (horizon split)
                call = lambda: ck(lib.pmenv_gae_ex(P(r), P(v), P(d), P(adv), P(ret), T, B, 0.99, 0.95,  # noqa: E731
                                                   P(work), nbytes, st), "gae")
                call()
                outs[mode] = (adv.clone(), ret.clone())
                us = timeit(call, a.reps)
                same_tile = bool(torch.equal(outs[mode][0], outs["tile"][0])) if "tile" in outs else None
                same_loop = bool(torch.equal(outs[mode][0], outs["loop"][0])) if "loop" in outs else None
                err = float((outs[mode][0] - outs["tile"][0]).abs().max()) if "tile" in outs else None
                res.append(row(f"gae_{mode}", us, alg, T=T, B=B, dones=dn, split=bool(nbytes) and mode == "auto",
                               same_bits_tile=same_tile, same_bits_loop=same_loop, max_abs_vs_tile=err))
            del outs
            for k in gk:
                os.environ.pop(k, None)
            del r, v, d, adv, ret
        # compact on-policy rollout: minibatch windows re-materialised from the resident
        # series + recorded w' (pmenv_rollout_gather), config 2's shape (4,096 envs x 32 steps)
        for Bc, Tr, S in ((4096, 32, 4096), (4096, 32, 32768), (65536, 64, 8192)):
            N_, W_ = 30, 50
            Ts = Tr + W_ + 8
            ser_c = torch.rand(Ts, N_, 4, device=dev, generator=g)
            start = torch.randint(0, 8, (Bc,), device=dev, generator=g).to(torch.int32)
            wts = torch.rand(Tr, Bc, N_, device=dev, generator=g)
            tix = torch.randint(0, Tr + 1, (S,), device=dev, generator=g).to(torch.int32)
            eix = torch.randint(0, Bc, (S,), device=dev, generator=g).to(torch.int32)
            out_c = torch.empty(S, N_, W_, 5, device=dev)
            call = lambda: ck(lib.pmenv_rollout_gather(P(ser_c), Ts, N_, 5, W_, P(start), P(wts), Tr, Bc, 0,  # noqa: E731
                                                       P(tix), P(eix), S, P(out_c), st), "rollout_gather")
            outs = {}
            # the product's LDS-staged tile, the wave-per-row and float-per-thread forms (tools)
            forms = (("tile", None), ("rows", "PMENV_RGATHER_ROWS"), ("elem", "PMENV_RGATHER_ELEM"),
                     ("tile_nt", "PMENV_RGATHER_NT=2"), ("tile_sc1", "PMENV_RGATHER_NT=16"),
                     ("tile_nt_sc1", "PMENV_RGATHER_NT=18"))
            for form, knob in forms:
                for k in ("PMENV_RGATHER_ELEM", "PMENV_RGATHER_ROWS", "PMENV_RGATHER_NT"):
                    os.environ.pop(k, None)
                if knob:
                    k, _, val = knob.partition("=")
                    os.environ[k] = val or "1"
                call()
                outs[form] = out_c.clone()
                res.append(row(f"rollout_gather_{form}", timeit(call, a.reps), S * N_ * W_ * 5 * 4, B=Bc, T=Tr, S=S,
                               N=N_, W=W_, same_bits=bool(torch.equal(outs[form], outs["tile"]))))
            for k in ("PMENV_RGATHER_ELEM", "PMENV_RGATHER_ROWS", "PMENV_RGATHER_NT"):
                os.environ.pop(k, None)
            del outs
            del ser_c, wts, out_c
        # advantage moments (the 24-byte all-reduce's input)
        for n in (256 * 65536, 256 * 4096):
            x = torch.randn(n, device=dev, generator=g)
            out = torch.empty(3, dtype=torch.float64, device=dev)
            work = torch.empty(lib.pmenv_moments_workspace() // 8, dtype=torch.float64, device=dev)
            us = timeit(lambda: ck(lib.pmenv_moments(P(x), n, P(out), P(work), st), "moments"), a.reps)
            res.append(row("moments", us, n * 4, n=n))

    if "f1" in only or "rollout_env" in only:
        # the compact rollout's per-env form (pmenv_rollout_gather_env) beside the lockstep gather
        # at config 2's buffer (4,096 envs x 32 steps, S = 4,096, N 30, W 50), same process, same
        # samples, alternating: fed the lockstep bookkeeping (first = start + t, updates = t; the
        # same bits), then envs that restart every 8-40 steps, each from its own phase. carry = W
        # with zero carry rows, as DeviceRolloutBuffer(episodes=True) holds them
        Bc, Tr, S, N_, W_ = 4096, 32, 4096, 30, 50
        Ts = Tr + W_ + 48
        ser_c = torch.rand(Ts, N_, 4, device=dev, generator=g)
        start = torch.randint(0, 8, (Bc,), device=dev, generator=g).to(torch.int32)
        wts = torch.rand(Tr, Bc, N_, device=dev, generator=g)
        wts_c = torch.cat([torch.zeros(W_, Bc, N_, device=dev), wts]).contiguous()
        tix = torch.randint(0, Tr + 1, (S,), device=dev, generator=g).to(torch.int32)
        eix = torch.randint(0, Bc, (S,), device=dev, generator=g).to(torch.int32)
        out_l, out_e = torch.empty(S, N_, W_, 5, device=dev), torch.empty(S, N_, W_, 5, device=dev)
        trow = torch.arange(Tr + 1, device=dev, dtype=torch.int32)[:, None]
        first_l = (start[None, :] + trow).contiguous()
        upd_l = trow.repeat(1, Bc).contiguous()
        length = torch.randint(8, 41, (Bc,), device=dev, generator=g).to(torch.int32)
        phase = (torch.rand(Bc, device=dev, generator=g) * length).to(torch.int32)
        upd_r = ((trow + phase[None, :]) % length[None, :]).contiguous()       # <= 39 < t + carry
        first_r = (start[None, :] + upd_r).contiguous()

        def lock(lib=lib):
            ck(lib.pmenv_rollout_gather(P(ser_c), Ts, N_, 5, W_, P(start), P(wts), Tr, Bc, 0, P(tix), P(eix), S,
                                        P(out_l), st), "rollout_gather")

        def env_form(first, upd):
            ck(lib.pmenv_rollout_gather_env(P(ser_c), Ts, N_, 5, W_, P(first), P(upd), P(wts_c), W_, Tr, Bc, 0,
                                            P(tix), P(eix), S, P(out_e), st), "rollout_gather_env")
        lock()
        env_form(first_l, upd_l)
        same = bool(torch.equal(out_l.view(torch.int32), out_e.view(torch.int32)))
        old = None
        if a.parent_lib:                       # the parent build's lockstep gather, same process
            old = ctypes.CDLL(a.parent_lib)
            old.pmenv_rollout_gather.restype, old.pmenv_rollout_gather.argtypes = next(
                (r, t) for n, r, t in _abi.SIGNATURES if n == "pmenv_rollout_gather")
            out_new = out_l.clone()
            out_l.zero_()
            lock(old)
            same_old = bool(torch.equal(out_l.view(torch.int32), out_new.view(torch.int32)))
        tl, te, tr_, tp = [], [], [], []
        for _ in range(5):
            tl.append(timeit(lock, a.reps))
            if old is not None:
                tp.append(timeit(lambda: lock(old), a.reps))
            te.append(timeit(lambda: env_form(first_l, upd_l), a.reps))
            tr_.append(timeit(lambda: env_form(first_r, upd_r), a.reps))
        base, us_e, us_r = statistics.median(tl), statistics.median(te), statistics.median(tr_)
        alg = S * N_ * W_ * 5 * 4
        kw = dict(B=Bc, T=Tr, S=S, N=N_, W=W_)
        res.append(row("rollout_gather_lockstep", base, alg, spread=round((max(tl) - min(tl)) / base, 4), **kw))
        if old is not None:
            us_p = statistics.median(tp)
            res.append(row("rollout_gather_lockstep_parent", us_p, alg, ratio_this_to_parent=round(base / us_p, 4),
                           spread=round((max(tp) - min(tp)) / us_p, 4), same_bits=same_old, **kw))
        res.append(row("rollout_gather_env", us_e, alg, ratio=round(us_e / base, 4),
                       spread=round((max(te) - min(te)) / us_e, 4), same_bits=same, **kw))
        res.append(row("rollout_gather_env_restarts", us_r, alg, ratio=round(us_r / base, 4),
                       spread=round((max(tr_) - min(tr_)) / us_r, 4),
                       restarts_per_env=round(float((upd_r[1:] == 0).float().sum(0).mean()), 2), **kw))
        del ser_c, wts, wts_c, out_l, out_e

    if "f2" in only:
        # differentiable batched PG reward: forward (reward only; the product's two launches
        # and the tools build's one-launch forms under PMENV_BR_ONE, interleaved) and backward
        for B, N in ((65536, 30), (16384, 30), (4096, 30), (8192, 500)):
            act = torch.randn(B, N, device=dev, generator=g)
            vp = torch.rand(B, device=dev, generator=g) + 1.0
            p = 1.0 + 0.01 * torch.randn(B, N, device=dev, generator=g)
            work = torch.empty(lib.pmenv_batch_reward_workspace(B) // 8, dtype=torch.float64, device=dev)
            rout = torch.empty((), device=dev)
            go = torch.ones((), device=dev)
            ga = torch.empty_like(act)
            fwd = lambda: ck(lib.pmenv_batch_reward_forward(P(act), P(vp), P(p), B, N, 0, 0, 1.0, P(work),  # noqa: E731
                                                            P(rout), None, st), "fwd")
            bwd = lambda: ck(lib.pmenv_batch_reward_backward(P(act), P(vp), P(p), B, N, 0, 1.0, P(work), P(go),  # noqa: E731
                                                             P(ga), st), "bwd")
            f_bytes = B * N * 4 * 2 + B * 4
            forms = {"two": {}, "one": {"PMENV_BR_ONE": "1"}, "one_fence_all": {"PMENV_BR_ONE": "1", "PMENV_BR_FENCE": "0"},
                     "one_grid256": {"PMENV_BR_ONE": "1", "PMENV_BR_GRID": "256"},
                     "one_grid512": {"PMENV_BR_ONE": "1", "PMENV_BR_GRID": "512"}}
            knobs = ("PMENV_BR_ONE", "PMENV_BR_FENCE", "PMENV_BR_GRID")

            def use(form):
                for k in knobs:
                    os.environ.pop(k, None)
                os.environ.update(forms[form])
            outs = {}
            for form in forms:                          # the same bits every way
                use(form)
                fwd()
                outs[form] = (rout.clone(), work[6 * B:6 * B + 5].clone())
            same = all(torch.equal(outs[f][0], outs["two"][0]) and torch.equal(outs[f][1], outs["two"][1])
                       for f in forms)
            ts = {f: [] for f in forms}
            for _ in range(3):
                for form in forms:
                    use(form)
                    ts[form].append(timeit(fwd, a.reps))
            use("two")
            for form in forms:
                res.append(row(f"batch_reward_fwd_{form}", statistics.median(ts[form]), f_bytes, B=B, N=N,
                               same_bits=same))
            res.append(row("batch_reward_bwd", timeit(bwd, a.reps), f_bytes + B * N * 4, B=B, N=N))

    if "f3" in only or "f4" in only:
        B, N, W, T = 65536, 30, 50, 512
        bars = synth.series(T, 1, N, device=dev)[:, 0].contiguous()
        ms = MarketSeries(bars, device=dev)
    if "f3" in only:
        # resident series: the env step with a per-env day index into one [T, N, 4] series
        starts = ms.random_starts(B, W, 64, generator=torch.Generator().manual_seed(1)).to(dev)
        obs = ms.initial_window(starts, W)
        out = torch.empty_like(obs)
        env = TradingEnv(num_envs=B, num_assets=N, window=W, device=dev)
        env.reset(obs)
        actn = synth.actions(1, B, N, device=dev)[0]
        day = starts.to(torch.int32) + W
        rew = torch.empty(B, device=dev)
        bufs = [obs, out]
        state = {"i": 0}
        args = _abi.PmenvStepArgs()
        args.action, args.bar, args.reward = actn.data_ptr(), ms.bars.data_ptr(), rew.data_ptr()
        args.day, args.series_days = day.data_ptr(), T

        def step_series(db):
            i = state["i"]
            args.obs = bufs[i % 2].data_ptr()
            args.obs_out = bufs[(i + 1) % 2].data_ptr() if db else None
            ck(lib.pmenv_step_ex(env._h, ctypes.byref(args), st), "step")
            if db:
                state["i"] = i + 1
        for db in (True, False):
            us = timeit(lambda: step_series(db), a.reps)
            res.append(row("step_resident_series", us, B * (8 * N * W * 5 + 20), B=B, N=N, W=W,
                           windows="double" if db else "inplace"))
        del obs, out, bufs, env
    if "f4" in only:
        # replay gather (S samples of s, s' windows) and trajectory metrics
        B, N, W, H, S = 4096, 30, 50, 256, 8192
        rb = DeviceReplay(B, N, W, H, ms)
        for h in range(H):
            rb.add(torch.full((B,), W + h, dtype=torch.int32, device=dev), torch.rand(B, N, device=dev),
                   torch.randn(B, device=dev))
        h0, e = rb.indices(S, generator=torch.Generator().manual_seed(2))
        s_ = torch.empty(S, N, W, 5, device=dev)
        s2 = torch.empty_like(s_)
        ao = torch.empty(S, N, device=dev)
        ro = torch.empty(S, device=dev)
        sb = ms.bars

        def gather():
            ck(lib.pmenv_replay_gather(P(sb), sb.shape[0], N, 5, W, P(rb.days), P(rb.actions), P(rb.rewards), H, B,
                                       P(h0), P(e), S, P(s_), P(s2), P(ao), P(ro), st), "gather")
        alg = S * (2 * N * W * 5 * 4 + N * 4 + 4)          # written windows dominate; reads hit L2
        for mode in ("f5", "lds"):
            os.environ.pop("PMENV_REPLAY_LDS", None)
            if mode == "lds":
                os.environ["PMENV_REPLAY_LDS"] = "1"
            res.append(row(f"replay_gather_{mode}", timeit(gather, a.reps), alg, S=S, N=N, W=W))
        os.environ.pop("PMENV_REPLAY_LDS", None)
        del rb
        # n-step gather beside the one-step gather at config 3's shape (16,384 envs x 30 x 50 x 5,
        # S = 8,192), same process, same indices: the one-step time and its repeats' spread,
        # then n = 1, 5, 64 as ratios to it
        B = 16384
        rb = DeviceReplay(B, N, W, H, ms)
        for h in range(H):
            rb.add(torch.full((B,), W + h, dtype=torch.int32, device=dev), torch.rand(B, N, device=dev),
                   torch.randn(B, device=dev))
        h0, e = rb.indices(S, generator=torch.Generator().manual_seed(2))
        stp = torch.empty(S, dtype=torch.int32, device=dev)
        dsc = torch.empty(S, device=dev)
        oldest = (rb.head - rb.count) % H

        def gather_n(n):
            ck(lib.pmenv_replay_gather_nstep(P(sb), sb.shape[0], N, 5, W, P(rb.days), P(rb.actions), P(rb.rewards),
                                             H, B, P(h0), P(e), S, P(rb._row_ep_dev), oldest, rb.count, n, 0.997,
                                             P(s_), P(s2), P(ao), P(ro), P(stp), P(dsc), st), "gather_nstep")
        reps1 = [timeit(gather, a.reps) for _ in range(5)]
        one = statistics.median(reps1)
        res.append(row("replay_gather_config3", one, alg, S=S, N=N, W=W, B=B,
                       spread=round((max(reps1) - min(reps1)) / one, 4)))
        for n in (1, 5, 64):
            us = statistics.median([timeit(lambda: gather_n(n), a.reps) for _ in range(5)])
            gather_n(n)
            res.append(row(f"replay_gather_nstep_n{n}", us, alg, S=S, N=N, W=W, B=B, n=n, ratio=round(us / one, 4),
                           mean_steps=round(float(stp.float().mean()), 2)))
        # sequence gather on the same ring beside the composition it replaces — the one-step
        # gather over the S*L pre-expanded indices (h0 + t, env), time-major, built outside the
        # timed region — same process, alternating: Dreamer's own batch (16 x 64) and 8,192
        # windows (128 x 64, as many as config 3's one-step s). Then the tools build's knobs:
        # the window stores' cache policy and the elements per chunk
        xq = torch.empty_like(s_)
        for Sq, L in ((16, 64), (128, 64)):
            Wn = Sq * L
            h0q, eq = rb.sequence_indices(Sq, L, generator=torch.Generator().manual_seed(3))
            tq = torch.arange(L, device=dev, dtype=torch.int32)[:, None]
            h0e = ((h0q[None, :] + tq) % H).reshape(-1).contiguous()
            ee = eq[None, :].expand(L, Sq).reshape(-1).contiguous()
            aq, rq = torch.empty(L, Sq, N, device=dev), torch.empty(L, Sq, device=dev)
            lq = torch.empty(Sq, dtype=torch.int32, device=dev)

            def composed():
                ck(lib.pmenv_replay_gather(P(sb), sb.shape[0], N, 5, W, P(rb.days), P(rb.actions), P(rb.rewards), H,
                                           B, P(h0e), P(ee), Wn, P(s_), P(s2), P(ao), P(ro), st), "gather")

            def seq():
                ck(lib.pmenv_replay_gather_seq(P(sb), sb.shape[0], N, 5, W, P(rb.days), P(rb.actions), P(rb.rewards),
                                               H, B, P(h0q), P(eq), Sq, P(rb._row_ep_dev), oldest, rb.count, L, 1,
                                               P(xq), P(aq), P(rq), P(lq), st), "gather_seq")
            knobs = ("PMENV_SEQ_NT", "PMENV_SEQ_LC")
            for k in knobs:
                os.environ.pop(k, None)
            composed()
            seq()
            same = bool(torch.equal(xq.view(-1)[:Wn * N * W * 5].view(torch.int32),
                                    s_.view(-1)[:Wn * N * W * 5].view(torch.int32)) and
                        torch.equal(aq.view(-1), ao.view(-1)[:Wn * N]) and torch.equal(rq.view(-1), ro[:Wn]) and
                        bool((lq == L).all()))
            tc, ts = [], []
            for _ in range(5):
                tc.append(timeit(composed, a.reps))
                ts.append(timeit(seq, a.reps))
            comp, us = statistics.median(tc), statistics.median(ts)
            alg_c = Wn * (2 * N * W * 5 * 4 + N * 4 + 4)
            alg_s = Wn * (N * W * 5 * 4 + N * 4 + 4)
            res.append(row(f"replay_gather_composed_S{Sq}_L{L}", comp, alg_c, S=Sq, L=L, N=N, W=W, B=B,
                           spread=round((max(tc) - min(tc)) / comp, 4)))
            res.append(row(f"replay_gather_seq_S{Sq}_L{L}", us, alg_s, S=Sq, L=L, N=N, W=W, B=B,
                           ratio=round(us / comp, 4), spread=round((max(ts) - min(ts)) / us, 4), same_bits=same,
                           frac_write_stream=round(alg_s / us / 1e6 / 4.24, 3)))
            if "libpmenv_ab" in os.path.basename(_abi.LIB_PATH):
                for k, vals in (("PMENV_SEQ_NT", (0, 2, 16)), ("PMENV_SEQ_LC", (1, 2, 4, 8, 16, 32))):
                    for v in vals:
                        os.environ[k] = str(v)
                        us_k = statistics.median([timeit(seq, a.reps) for _ in range(3)])
                        res.append(row(f"replay_gather_seq_S{Sq}_L{L}_{k[6:].lower()}{v}", us_k, alg_s, S=Sq, L=L,
                                       ratio=round(us_k / comp, 4)))
                    os.environ.pop(k, None)
        del rb, s_, s2, xq
        for T, B in ((252, 65536), (252, 4096)):
            rets = 0.001 * torch.randn(T, B, device=dev, dtype=torch.float64, generator=g)
            vals = torch.cumprod(torch.cat([torch.ones(1, B, device=dev, dtype=torch.float64), 1 + rets]), 0)
            wts = torch.softmax(torch.randn(T + 1, B, 30, device=dev, generator=g), -1)
            out = torch.empty(B, 5, dtype=torch.float64, device=dev)
            alg = T * B * 8 + (T + 1) * B * 8 + (T + 1) * B * 30 * 4 + B * 5 * 8
            for mode in ("fused", "seg", "walk"):
                os.environ.pop("PMENV_METRICS_WALK", None)
                os.environ.pop("PMENV_METRICS_FUSED", None)
                if mode == "walk":
                    os.environ["PMENV_METRICS_WALK"] = "1"
                if mode == "seg":                       # the two passes as two launches
                    os.environ["PMENV_METRICS_FUSED"] = "0"
                us = timeit(lambda: ck(lib.pmenv_metrics(P(rets), P(vals), P(wts), T, B, 30, 0.04, 252.0, P(out), st),
                                       "metrics"), a.reps)
                res.append(row(f"trajectory_metrics_{mode}", us, alg, T=T, B=B, N=30))
            os.environ.pop("PMENV_METRICS_WALK", None)
            os.environ.pop("PMENV_METRICS_FUSED", None)

    if "prio" in only:
        # the priority tree on config 3's ring (L = 16,384 envs x 256 rows) beside the torch
        # statement of the same work on a bare f32 priority array, same process, alternating:
        # the draw is cumsum in f64 over every leaf + searchsorted + the weights; the update
        # a pow and a scatter with amax (no tree to maintain: its cost is the draw's cumsum);
        # the fill two slice assignments. S = 256 is config's batch, 8,192 the gather row's size
        from pmenv.replay import prio_layout, prio_tree
        Bp, Hp = 16384, 256
        Lp = Bp * Hp
        lay = prio_layout(Lp)
        tree = prio_tree(Lp, dev)
        ck(lib.pmenv_prio_fill(P(tree), Lp, -1, 0, Lp, st), "prio_fill")
        ck(lib.pmenv_prio_fill(P(tree), Lp, 17 * Bp, -1, 5 * Bp, st), "prio_fill")       # some closed rows
        seed_idx = torch.randint(0, Lp, (1 << 20,), device=dev, generator=g, dtype=torch.int32)
        seed_td = torch.randn(1 << 20, device=dev, generator=g) * 3
        ck(lib.pmenv_prio_update(P(tree), Lp, P(seed_idx), P(seed_td), 1 << 20, 0.6, 1e-6, st), "prio_update")
        leaves_t = tree[64:64 + 4 * Lp].view(torch.float32).clone()                        # the torch side's array
        nlev = len(lay["levels"]) - 1

        def both(name, hip, ref, alg, **kw):
            hip()
            ref()
            th, tr = [], []
            for _ in range(5):
                th.append(timeit(hip, a.reps))
                tr.append(timeit(ref, a.reps))
            us, base = statistics.median(th), statistics.median(tr)
            res.append(row(name + "_torch", base, alg, spread=round((max(tr) - min(tr)) / base, 4), **kw))
            res.append(row(name, us, alg, ratio=round(us / base, 4), spread=round((max(th) - min(th)) / us, 4),
                           baseline="torch: " + kw.get("torch", ""), **{k: v for k, v in kw.items() if k != "torch"}))

        for Sp in (256, 8192):
            u = ((torch.arange(Sp, device=dev, dtype=torch.float64) +
                  torch.rand(Sp, device=dev, dtype=torch.float64, generator=g)) / Sp).contiguous()
            lo, ho, eo = (torch.empty(Sp, dtype=torch.int32, device=dev) for _ in range(3))
            wo = torch.empty(Sp, device=dev)
            td = torch.randn(Sp, device=dev, generator=g)
            got = {}

            def sample():
                ck(lib.pmenv_prio_sample(P(tree), Lp, Bp, P(u), Sp, 0.4, P(lo), P(ho), P(eo), P(wo), st), "prio_sample")

            def sample_torch():
                c = torch.cumsum(leaves_t.double(), 0)
                i = torch.searchsorted(c, u * c[-1], right=True).clamp_(max=Lp - 1)
                pv = leaves_t[i]
                got["i"], got["w"] = i, (pv.double() / pv.min().double()).pow(-0.4).float()
            both(f"prio_sample_S{Sp}", sample, sample_torch, Sp * (nlev * 512 + 256 + 8 + 16), S=Sp, L=Lp,
                 torch="cumsum f64 over the leaves + searchsorted + weights")
            res[-1]["same_leaves"] = round(float((got["i"].to(torch.int32) == lo).float().mean()), 4)

            def update():
                ck(lib.pmenv_prio_update(P(tree), Lp, P(lo), P(td), Sp, 0.6, 1e-6, st), "prio_update")
            li = lo.long()

            def update_torch():
                leaves_t.scatter_reduce_(0, li, (td.abs().double() + 1e-6).pow(0.6).float(), "amax", include_self=False)
            both(f"prio_update_S{Sp}", update, update_torch, Sp * (8 + nlev * 520 + 256), S=Sp, L=Lp,
                 torch="pow + scatter_reduce amax on the bare array (no tree)")
        state = {"h": 0}

        def fill():
            h = state["h"]
            state["h"] = (h + 1) % Hp
            ck(lib.pmenv_prio_fill(P(tree), Lp, h * Bp, ((h + 100) % Hp) * Bp, Bp, st), "prio_fill")

        def fill_torch():
            h = state["h"]
            state["h"] = (h + 1) % Hp
            leaves_t[h * Bp:(h + 1) * Bp] = 0.0
            o = (h + 100) % Hp
            leaves_t[o * Bp:(o + 1) * Bp] = 1.0
        both("prio_fill_B16384", fill, fill_torch, 2 * Bp * 4 * 2 + 2 * (Bp // 64) * 8, n=Bp, L=Lp,
             torch="two slice assignments on the bare array (no tree)")
        del tree, leaves_t

    doc = {"device": torch.cuda.get_device_name(0), "peak_GBs": PEAK_GBS, "cases": res}
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
