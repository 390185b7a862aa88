"""The compact rollout's per-env form on the host: DeviceRolloutBuffer(episodes=True)'s
first / updates / done bookkeeping and resume() against a per-env Python simulation (host
tensors, Episodes.advance_host in place of the restart kernel), pmenv_rollout_gather_env_path
against pmenv_replay_path over the plan sweep's rollout shapes, and the kernels it names
against the library's device stubs (no GPU)."""
import itertools
import re
import subprocess

import numpy as np
import pytest
import torch

from pmenv import _abi
from test_replay_plan_host import ALIGNED, CUS, FS, NS, SS, WS

ENV_NAMES = {"rollout_gather_tile_kernel": "rollout_gather_env_tile_kernel",
             "rollout_gather_rows_kernel": "rollout_gather_env_rows_kernel"}


def simulate(start, restart, length, W, steps):
    """Per env, one at a time: (first, updates, done) [steps + 1] of the windows the env holds
    after 0 .. steps steps, each followed by the restart call."""
    B = len(start)
    first = np.zeros((steps + 1, B), np.int64)
    upd = np.zeros((steps + 1, B), np.int64)
    done = np.zeros((steps + 1, B), np.int64)
    for b in range(B):
        f, u, end = start[b], 0, start[b] + W + length[b]
        first[0, b] = f
        for t in range(1, steps + 1):
            appended = f + W                       # the bar step t appends
            if appended + 1 >= end:                # the episode's last bar: restart
                f, u, end = restart[b], 0, restart[b] + W + length[b]
                done[t, b] = 1
            else:
                f, u = f + 1, u + 1
            first[t, b], upd[t, b] = f, u
    return first, upd, done


@pytest.mark.parametrize("T", [3, 9])          # T < W and T > W
def test_bookkeeping_and_resume_against_a_per_env_simulation(T):
    from pmenv import MarketSeries
    from pmenv.episodes import Episodes
    from pmenv.rollout_buffer import DeviceRolloutBuffer
    B, N, W, rounds = 7, 3, 5, 3
    days = 80
    rng = np.random.default_rng(T)
    start = np.array([0, 3, 9, 4, 11, 2, 20])
    restart = np.array([5, 3, 0, 30, 11, 7, 1])
    length = np.array([1, W - 1, W, W + 3, T, 60, 2 * T])
    m = MarketSeries(rng.random((days, N, 4)).astype(np.float32), device="cpu")
    ep = Episodes(days, W, start, restart=restart, length=length, device="cpu")
    buf = DeviceRolloutBuffer(B, N, W, T, device="cpu", series=m, episodes=True)
    assert buf.w.shape == (W + T, B, N) and buf.carry == W
    assert buf.first.shape == buf.updates.shape == buf.done.shape == (T + 1, B)
    assert buf.first.dtype == buf.updates.dtype == torch.int32 and buf.done.dtype == torch.uint8
    held = sum(x.numel() * x.element_size() for x in (buf.a, buf.v, buf.r, buf.start, buf.w, buf.first, buf.updates,
                                                      buf.done))
    assert buf.nbytes() == held
    first, upd, done = simulate(start, restart, length, W, rounds * T)
    assert done[:, 0].sum() == rounds * T and done[:, 5].sum() == 0           # length 1; never restarts
    assert done[T, 4] == 1                                                    # ends exactly at step T
    hist = [np.zeros((B, N), np.float32)] * W                                 # w' of every step, W zero rows in front
    acts, vals = [], []
    buf.reset(start=torch.as_tensor(start))
    for k in range(rounds):
        if k:
            buf.resume()
            assert len(buf) == 0
            # the carry rows: the last W history rows; row 0: the last row of the rollout before
            assert np.array_equal(buf.w[:W].numpy(), np.stack(hist[-W:]))
            assert np.array_equal(buf.a[0].numpy(), acts[-1]) and np.array_equal(buf.v[0].numpy(), vals[-1])
            assert float(buf.r[0].abs().sum()) == 0.0
        else:
            assert float(buf.w.abs().sum()) == 0.0 and buf.a[0, :, 0].tolist() == [1.0] * B
        for t in range(1, T + 1):
            g = k * T + t
            a = torch.as_tensor(rng.random((B, N)).astype(np.float32))
            wp = torch.as_tensor(rng.random((B, N)).astype(np.float32))
            v = torch.as_tensor(rng.random(B))
            buf.add(a, v, torch.full((B,), float(g)), weights=wp)
            with pytest.raises(RuntimeError):
                buf.add(a, v, torch.zeros(B), weights=wp)                     # the restart was not recorded yet
            buf.restarted(ep.advance_host(), ep.next_day)
            hist.append(wp.numpy())
            acts.append(a.numpy())
            vals.append(v.numpy())
            assert np.array_equal(buf.w[W + t - 1].numpy(), hist[-1])
        lo = k * T
        assert np.array_equal(buf.first.numpy(), first[lo:lo + T + 1]), k
        assert np.array_equal(buf.updates.numpy(), upd[lo:lo + T + 1]), k
        assert np.array_equal(buf.done[1:].numpy(), done[lo + 1:lo + T + 1]), k
        assert np.array_equal(buf.w.numpy(), np.stack(hist[-(W + T):]))
        assert buf.r[1:, 0].tolist() == [float(lo + t) for t in range(1, T + 1)]
    with pytest.raises(IndexError):
        buf.add(a, v, torch.zeros(B), weights=wp)


def test_episodes_need_the_compact_form():
    from pmenv.rollout_buffer import DeviceRolloutBuffer
    with pytest.raises(ValueError, match="series"):
        DeviceRolloutBuffer(2, 3, 4, 5, device="cpu", episodes=True)


def test_env_path_is_the_rollout_path_with_the_env_kernels_names():
    lib = _abi.load()
    seen = set()
    for N, W, F, S, al in itertools.product(NS, WS, FS, SS + (4096, 32768), ALIGNED):
        lock = lib.pmenv_replay_path(_abi.REPLAY_KINDS["rollout"], N, F, W, 1, S, al, CUS).decode()
        name = lock.split("_kernel")[0] + "_kernel"
        want = lock.replace(name, ENV_NAMES[name], 1)
        assert lib.pmenv_rollout_gather_env_path(N, F, W, S, al).decode() == want, (N, W, F, S, al)
        seen.add(want.split(" ")[0])
    assert seen == {"rollout_gather_env_tile_kernel<16>", "rollout_gather_env_tile_kernel<2>",
                    "rollout_gather_env_rows_kernel"}
    ok = (30, 5, 50, 64, 3)
    assert lib.pmenv_rollout_gather_env_path(*ok) == b"rollout_gather_env_tile_kernel<16> R=0 grid=64x1 lds=30000"
    for i, bad in ((0, 0), (1, 1), (2, 0), (3, 0), (4, 4), (4, -1)):
        assert lib.pmenv_rollout_gather_env_path(*ok[:i], bad, *ok[i + 1:]) == b"", (i, bad)


def test_every_named_env_kernel_is_in_the_library_beside_the_lockstep_ones():
    lib = _abi.load()
    syms = subprocess.run(["nm", "-C", _abi.LIB_PATH], capture_output=True, text=True).stdout
    stubs = {m.replace(" ", "") for m in re.findall(r"__device_stub__(\w+(?:<[^>]*>)?)\(", syms)}
    assert stubs, "no kernel stubs found"
    names = {lib.pmenv_rollout_gather_env_path(N, F, W, S, al).decode().split(" ")[0]
             for N, W, F, S, al in itertools.product(NS, WS, FS, SS + (4096, 32768), ALIGNED)}
    assert len(names) == 3 and names <= stubs, f"named but not instantiated: {sorted(names - stubs)}"
    assert {"rollout_gather_tile_kernel<16>", "rollout_gather_rows_kernel"} <= stubs
