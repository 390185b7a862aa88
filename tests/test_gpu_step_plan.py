"""The handle and the device-less plan agree: for every step_impl, a fresh handle's
pmenv_step_path is pmenv_step_path_for's string for its cfg (csrc/step_plan.h serves both), a
path pmenv_set_step_path refuses is "" there, and a step enqueued under stream capture adds
only the device-sequenced note, which belongs to the handle's history. Needs an MI355X."""
import ctypes

import pytest
import torch

from test_gpu_parity import DEV, _gpu  # noqa: F401  (_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

# (B, N, W, F, extra cfg): tiny, one workgroup per env, not 16-B granular, the generic stream
# below and above its threshold, wide envs, the relay band (51 MB), four envs per tile
SHAPES = [
    (1, 5, 50, 5, {}),
    (64, 30, 50, 5, {}),
    (64, 30, 50, 5, {"commission": 0.0025}),
    (41, 7, 6, 3, {}),
    (128, 30, 50, 8, {}),
    (16, 30, 50, 12, {}),
    (256, 65, 50, 5, {}),
    (24, 200, 50, 5, {}),
    (1700, 30, 50, 5, {}),
    (800, 8, 50, 5, {}),
    (5, 30, 50, 5, {}),
    (7, 513, 3, 5, {}),
]


@pytest.mark.parametrize("B,N,W,F,kw", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" + ("c" if s[4] else "") for s in SHAPES])
def test_gpu_handle_path_is_the_deviceless_plan(B, N, W, F, kw):
    from pmenv import TradingEnv, _abi, step_path_for
    kw = dict(kw, close_channel=min(3, F - 2))
    env = TradingEnv(num_envs=B, num_assets=N, window=W, features=F, device=DEV, **kw)
    fitted = 0
    for impl in _abi.STEP_PATHS:
        want = step_path_for(env.cfg, impl)
        assert " -- " not in want and step_path_for(env.cfg, impl, detail=True).startswith(want + " -- " if want else "")
        before = env.step_path
        if want == "":
            with pytest.raises(ValueError):
                env.set_step_impl(impl)
            assert env.step_path == before                       # refused: the handle keeps its path
        else:
            env.set_step_impl(impl)
            assert env.step_path == want, impl
            fitted += 1
    assert fitted >= 1                                           # AUTO fits every shape
    assert step_path_for(num_envs=B, num_assets=N, window=W, features=F, **kw) == step_path_for(env.cfg)
    env.close()


@pytest.mark.parametrize("impl,note", [("flat", " [flat steps device-sequenced]"),
                                       ("relay", " [relay steps device-sequenced]")])
def test_gpu_captured_step_adds_only_the_sequencing_note(impl, note):
    from pmenv import TradingEnv, _abi, step_path_for, synth
    B, N, W = 64, 30, 50
    lib = _abi.load()
    ser = synth.series(W + 2, B, N, seed=5, device=DEV)
    act = synth.actions(2, B, N, seed=6, device=DEV)
    env = TradingEnv(num_envs=B, num_assets=N, window=W, device=DEV, step_impl=impl)
    ref = TradingEnv(num_envs=B, num_assets=N, window=W, device=DEV, step_impl="two_launch")
    obs, obs_ref = synth.window_from_series(ser, W), synth.window_from_series(ser, W)
    env.reset(obs)
    ref.reset(obs_ref)
    plain = step_path_for(env.cfg, impl)
    assert env.step_path == plain and "device-sequenced" not in plain
    a, bar, rew = act[0].clone(), ser[W].clone(), torch.empty(B, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _abi.check(lib.pmenv_step(env._h, p(a), None, p(bar), p(obs), p(rew), s), env._h)
    assert env.step_path == plain + note
    g.replay()
    r_ref, _ = ref.step(act[0], obs_ref, bar=ser[W])
    torch.cuda.synchronize()
    assert torch.equal(rew, r_ref) and torch.equal(obs, obs_ref)
    env.set_step_impl("two_launch")                              # the note names steps the handle takes now
    assert env.step_path == step_path_for(env.cfg, "two_launch")
