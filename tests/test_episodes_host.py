"""pmenv.episodes.Episodes on host tensors: the constructor's checks, the defaults, the day
convention and the `length` update of `end` (no GPU)."""
import re

import numpy as np
import pytest
import torch

from episode_ref import restart_ref, window_ref

DAYS, W = 100, 10


def _ep(**kw):
    from pmenv.episodes import Episodes
    kw.setdefault("start", [0, 5, 20])
    return Episodes(DAYS, W, device="cpu", **kw)


@pytest.mark.parametrize("kw,env,what", [
    (dict(start=[0, -1, 3]), 1, "start must be >= 0"),
    (dict(restart=[0, 5, -2]), 2, "restart must be in"),
    (dict(restart=[DAYS - W + 1, 5, 20]), 0, "restart must be in"),
    (dict(end=[50, 50, DAYS + 1]), 2, "end must be <="),
    (dict(restart=[0, 40, 20], end=[50, 50, 50]), 1, "restart + window must be < end"),
    (dict(start=[0, 5, 40], restart=[0, 5, 20], end=[50, 50, 50]), 2, "start + window must be < end"),
    (dict(length=[5, 0, 5]), 1, "length must be at least 1"),
    (dict(restart=[0, 5, 88], length=3), 2, "restart + window + length"),
])
def test_constructor_names_the_first_bad_env(kw, env, what):
    with pytest.raises(ValueError, match=f"env {env}: .*{re.escape(what)}"):
        _ep(**kw)


def test_constructor_boundaries_are_accepted():
    ep = _ep(start=[0, 89], restart=[0, 89], end=[11, DAYS])            # start + W + 1 == end; end == days
    assert ep.end.tolist() == [11, DAYS]


def test_end_and_length_exclude_each_other():
    with pytest.raises(ValueError, match="exclude"):
        _ep(end=[50, 50, 50], length=4)
    with pytest.raises(ValueError, match="one value per env"):
        _ep(end=[50, 50])


def test_defaults():
    ep = _ep()
    assert ep.end.tolist() == [DAYS] * 3                                # the series' end: the reference's episode
    assert ep.restart.tolist() == [0, 5, 20]                            # restart = start
    assert ep.done.dtype == torch.uint8 and ep.done.tolist() == [0, 0, 0]
    for t in (ep.next_day, ep.end, ep.restart):
        assert t.dtype == torch.int32 and t.shape == (3,)
    days_from_tensor = type(ep)(torch.zeros(DAYS, 4, 3), W, [1], device="cpu")
    assert days_from_tensor.end.tolist() == [DAYS]


def test_day_convention_first_step_appends_start_plus_window():
    ep = _ep()
    assert ep.day.tolist() == [W - 1, W + 4, W + 19]                    # the latest bar in the window
    assert ep.next_day.tolist() == [W, W + 5, W + 20]                   # what step(day=) takes: day + 1
    nd = ep.next_day
    ep.advance_host()
    assert ep.next_day is nd and ep.next_day.tolist() == [W + 1, W + 6, W + 21]


def test_length_update_of_end_over_three_restarts():
    start = np.array([0, 5, 20, 7])
    restart = np.array([30, 0, 20, 50])
    length = np.array([3, 5, 4, 6])
    ep = _ep(start=start, restart=restart, length=length)
    day, end = start + W, start + W + length
    assert ep.end.tolist() == end.tolist()
    done_t = ep.done
    counts = np.zeros(4, int)
    for _ in range(3 * 6 + 1):
        done, day = restart_ref(day, end, restart, W)
        end = np.where(done, restart + W + length, end)
        got = ep.advance_host()
        assert got is done_t
        assert got.bool().tolist() == done.tolist()
        assert ep.next_day.tolist() == day.tolist()
        assert ep.end.tolist() == end.tolist()
        counts += done
    assert (counts >= 3).all()
    # every episode is `length` steps long: env 0 ends on steps 3, 6, 9, ...
    assert counts[0] == 19 // 3


def test_fixed_end_is_kept_across_restarts():
    ep = _ep(start=[0, 5, 20], restart=[1, 80, 80], end=[12, 95, 95])
    ep.advance_host()
    assert ep.done.tolist() == [0, 0, 0]
    ep.advance_host()
    assert ep.done.tolist() == [1, 0, 0] and ep.next_day.tolist() == [11, 17, 32]
    assert ep.end.tolist() == [12, 95, 95]


def test_refs():
    done, day = restart_ref([10, 11, 12], [12, 12, 20], [3, 4, 5], 6)
    assert done.tolist() == [False, True, False] and day.tolist() == [11, 10, 13]
    ser = np.arange(5 * 2 * 2, dtype=np.float32).reshape(5, 2, 2)
    w = window_ref(ser, [1, 3, -1], 3, 3)
    assert w.shape == (3, 2, 3, 3)
    assert np.array_equal(w[0, :, :, :2], ser[1:4].transpose(1, 0, 2))
    assert w[0, 0, 2, 2] == 1 and w[0, :, :, 2].sum() == 1
    assert np.isnan(w[1, :, 2, :2]).all() and not np.isnan(w[1, :, :2, :2]).any()
    assert np.isnan(w[2, :, :, :2]).all()
