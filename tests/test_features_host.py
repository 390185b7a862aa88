"""The feature pipeline's host side (no GPU): the numpy restatements the GPU tests compare
the kernels with (tests/ffd_ref.py) against the reference's own outputs in tests/golden/
ffd/ffd_*.npz, MarketSeries(relatives=)'s shape checks, and the compact rollout buffer's p taken
from the series' table (host tensors; the window gather stubbed out).

The bounds. FFD: width * 2^-24 * sum_j |w_j x_{t-j}| + ulp32, the worst case of the
reference's own f32 dot product in any order against the exact sum (the restatement is the
exact sum rounded once). Scalers: 8 * 2^-24 * (|x| + |min or mean|) / (range or std) +
2^-24 * max(1, |y|), counting sklearn's f32 roundings of scale_, min_, the product and the sum."""
import numpy as np
import pytest
import torch

import ffd_ref
from ffd_ref import golden, golden_taps, table_of


@pytest.mark.parametrize("name", ["mixed_t600", "t6000"])
def test_ffd_restatement_reproduces_the_reference_transform(name):
    g = golden(name)
    x = g["raw"][1:]
    table, widths = table_of(golden_taps(g))
    assert np.array_equal(widths, g["widths"]) and int(g["max_width"]) == table.shape[0]
    out = ffd_ref.ffd_ref(x, table, widths, table.shape[0])
    assert out.shape == g["ffd"].shape
    bound = ffd_ref.ffd_bound(x, table, widths, table.shape[0], g["ffd"])
    err = np.abs(out.astype(np.float64) - g["ffd"].astype(np.float64))
    print(f"{name}: largest error / bound = {(err / bound).max():.3g}")
    assert np.all(err <= bound)
    for c in np.flatnonzero(widths == 0):                     # a column left alone: the same bits
        assert np.array_equal(out[:, c].view(np.uint32), x[table.shape[0]:, c].view(np.uint32))


def test_ffd_restatement_identity_and_nan_confinement():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(40, 3)).astype(np.float32)
    taps = [np.array([1.0], np.float32), rng.normal(size=5).astype(np.float32), np.zeros(0, np.float32)]
    table, widths = table_of(taps)
    base = ffd_ref.ffd_ref(x, table, widths, 5)
    assert np.array_equal(base[:, 0], x[5:, 0]) and np.array_equal(base[:, 2], x[5:, 2])   # d = 1 and d = 0
    x[20, 1] = np.nan
    out = ffd_ref.ffd_ref(x, table, widths, 5)
    assert np.flatnonzero(np.isnan(out[:, 1])).tolist() == list(range(15, 20))             # rows 20 .. 24 of x
    keep = ~np.isnan(out)
    assert np.array_equal(out[keep].view(np.uint32), base[keep].view(np.uint32))


@pytest.mark.parametrize("method", ["minmax", "standard"])
def test_scaler_restatement_reproduces_sklearn(method):
    g = golden("mixed_t600")
    split, purge = int(g["split"]), int(g["purge"])
    assert split == int(0.8 * len(g["ffd"])) and purge == int(g["max_width"])
    worst = 0.0
    for part, rows in (("train", g["ffd"][:split]), ("test", g["ffd"][split + purge:])):
        want = g[f"{part}_{method}"]
        assert want.shape == rows.shape
        y, stats = ffd_ref.scale_ref(rows, method)
        bound = ffd_ref.scale_bound(rows, y, stats, method)
        err = np.abs(y.astype(np.float64) - want.astype(np.float64))
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (part, float((err / bound).max()))
    print(f"{method}: largest error / bound = {worst:.3g}")


def test_scaler_restatement_edge_columns():
    x = np.stack([np.full(9, 3.5), np.r_[1.0, np.nan, 3.0, np.zeros(6)], 1000.0 + 0.25 * np.r_[-1, 1, -1, 1, 0, 0, 1, -1, 0],
                  np.r_[-0.0, 0.0, -0.0, np.zeros(6)]], axis=1).astype(np.float32)
    for method in ("minmax", "standard"):
        y, stats = ffd_ref.scale_ref(x, method)
        assert np.all(y[:, 0] == 0.0) and np.all(y[:, 3] == 0.0)          # constant: divides by 1
        assert np.isnan(y[1, 1]) and np.isfinite(np.delete(y[:, 1], 1)).all()
    y, stats = ffd_ref.scale_ref(x, "minmax")
    assert stats[:, 1].tolist() == [0.0, 3.0] and stats[:, 2].tolist() == [999.75, 1000.25]
    assert y[:, 2].min() == 0.0 and y[:, 2].max() == 1.0
    y, stats = ffd_ref.scale_ref(x, "standard")
    assert stats[0, 2] == 1000.0 and abs(stats[1, 2] - 0.25 * np.sqrt(6 / 9)) < 1e-15


# ---------------------------------------------------------------- MarketSeries(relatives=)
def test_market_series_relatives_shape_checks():
    from pmenv import MarketSeries
    bars = np.random.default_rng(1).random((12, 3, 4)).astype(np.float32)
    rel = np.random.default_rng(2).random((12, 3)).astype(np.float32) + 0.5
    m = MarketSeries(bars, device="cpu")
    assert m.relatives is None
    m = MarketSeries(bars, device="cpu", relatives=rel)
    assert m.relatives.shape == (12, 3) and m.relatives.dtype == torch.float32 and m.relatives.is_contiguous()
    assert np.array_equal(m.relatives.numpy(), rel)
    m64 = MarketSeries(bars, device="cpu", relatives=torch.as_tensor(rel.astype(np.float64)).t().contiguous().t())
    assert m64.relatives.dtype == torch.float32 and m64.relatives.is_contiguous()
    for bad in (rel[:11], rel[:, :2], rel[None], rel.reshape(-1), np.zeros((13, 3), np.float32)):
        with pytest.raises(ValueError):
            MarketSeries(bars, device="cpu", relatives=bad)
    got = m.relatives_at(torch.tensor([0, 11, -1, 12, 5], dtype=torch.int32))
    assert np.array_equal(got[[0, 1, 4]].numpy(), rel[[0, 11, 5]])
    assert torch.isnan(got[2]).all() and torch.isnan(got[3]).all()       # a day outside [0, T), as the bar reads


# ---------------------------------------------------------------- the compact buffer's p
@pytest.mark.parametrize("episodes", [False, True])
def test_rollout_buffer_takes_p_from_the_series_table(episodes, monkeypatch):
    from pmenv import MarketSeries
    from pmenv.episodes import Episodes
    from pmenv.rollout_buffer import DeviceRolloutBuffer
    B, N, W, T, days = 5, 3, 4, 9, 60
    rng = np.random.default_rng(3)
    bars = rng.random((days, N, 4)).astype(np.float32) + 0.5
    rel = rng.random((days, N)).astype(np.float32) + 0.5
    start = np.array([0, 3, 9, 4, 11])
    plain = MarketSeries(bars, device="cpu")
    table = MarketSeries(bars, device="cpu", relatives=rel)
    bufs = {}
    for key, series in (("plain", plain), ("table", table)):
        buf = DeviceRolloutBuffer(B, N, W, T, device="cpu", series=series, episodes=episodes)
        buf.reset(start=torch.as_tensor(start))
        ep = Episodes(days, W, start, restart=np.array([5, 3, 0, 30, 11]), length=np.array([1, 3, 4, 7, 40]),
                      device="cpu")
        days_read = []
        for t in range(1, T + 1):
            a = torch.as_tensor(rng.random((B, N)).astype(np.float32))
            days_read.append(ep.next_day.clone().long() if episodes else torch.as_tensor(start + W + t - 1))
            buf.add(a, torch.ones(B, dtype=torch.float64), torch.zeros(B), weights=a)
            if episodes:
                buf.restarted(ep.advance_host(), ep.next_day)
        bufs[key] = (buf, days_read)
    buf, days_read = bufs["table"]
    pbuf, _ = bufs["plain"]
    for t in range(1, T + 1):
        day = days_read[t - 1]
        assert np.array_equal(buf.price_relatives(t).numpy(), rel[day.numpy()])          # the row the step read
        want = bars[day.numpy(), :, 3] / bars[day.numpy() - 1, :, 3]                     # without a table: as before
        assert np.array_equal(pbuf.price_relatives(t).numpy(), want)
    # gather's p, the window gather stubbed out (its kernels need a device)
    def stub(b):
        def windows(t, env):
            last = bars[b._last_day(t.long(), env.long()).numpy()]                        # [S, N, 4]
            win = np.zeros((len(last), N, W, 5), np.float32)
            win[:, :, W - 1, :4] = last
            return torch.as_tensor(win)
        return windows
    for b in (buf, pbuf):
        monkeypatch.setattr(b, "windows", stub(b))
    steps = torch.tensor([1, 4, 9, 2, 7])
    envs = torch.tensor([0, 1, 2, 3, 4])
    p = buf.gather(steps, envs)[5]
    want = np.stack([rel[days_read[int(t) - 1][int(e)]] for t, e in zip(steps, envs)])
    assert p.shape == (5, N, 1) and np.array_equal(p[..., 0].numpy(), want)
    p0 = pbuf.gather(steps, envs)[5]                                                      # close / the window's last close
    assert p0.shape == (5, N, 1) and not np.array_equal(p0.numpy(), p.numpy())
