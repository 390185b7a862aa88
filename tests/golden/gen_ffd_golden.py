"""Golden fixtures of the feature pipeline: tests/golden/ffd/ffd_*.npz (a folder of their own: the env goldens' loader
takes every .npz directly under tests/golden for one of its cases).

Run in the build container only: it loads the reference's data/ffd.py at run time (nothing
of it is copied here) and runs its FixedFracDiff on the CPU, then sklearn's MinMaxScaler and
StandardScaler as data/instrument.py:318-336 applies them, per column. The two packages
ffd.py imports but the fixtures do not need are stubbed: tensordict.TensorDict (a dict of
equally long 1-D tensors with `to`, `len`, `keys` and row slicing) and
statsmodels.tsa.stattools.adfuller (a constant p-value: every column here comes with its d,
as from the reference's d_opt pickles, so the search for one never runs; an order of 0 can
only be had through the reference's ignore list, its search fails on an empty filter).

A case follows one ticker through the loader's order (data/instrument.py:79-80, 257-336):

    raw [T+1, C]        the market channels, close among them
    relatives [T]       close[1:] / close[:-1]
    x = raw[1:]         the features the differencing sees, [T, C]
    d [C], thres        the orders (0: left alone; `volume` sits in the reference's ignore list)
    taps, widths        the reference's weights, tap 0 first, concatenated over the columns,
                        and their widths; max_width
    ffd [T - max_width, C]   FixedFracDiff.transform
    split, purge        int(0.8 * len) and max_width (instrument.py:303-313)
    train_minmax, test_minmax, train_standard, test_standard   each part scaled on its own

    python tests/golden/gen_ffd_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference
REF = os.environ.get("PMRL_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))


class TensorDict(dict):
    """The little of tensordict.TensorDict that data/ffd.py touches."""

    def __init__(self, source=None, **_):
        super().__init__(source or {})

    def to(self, device):
        return TensorDict({k: v.to(device) for k, v in self.items()})

    def __len__(self):
        return len(next(iter(self.values()))) if dict.__len__(self) else 0

    def __getitem__(self, key):
        if isinstance(key, slice):
            return TensorDict({k: v[key] for k, v in self.items()})
        return dict.__getitem__(self, key)


def load_ffd():
    td = types.ModuleType("tensordict")
    td.TensorDict = TensorDict
    sm, tsa, st = (types.ModuleType(n) for n in ("statsmodels", "statsmodels.tsa", "statsmodels.tsa.stattools"))
    st.adfuller = lambda series, *a, **k: (0.0, 0.04)
    sm.tsa, tsa.stattools = tsa, st
    sys.modules.update({"tensordict": td, "statsmodels": sm, "statsmodels.tsa": tsa, "statsmodels.tsa.stattools": st})
    spec = importlib.util.spec_from_file_location("ref_ffd", os.path.join(REF, "data", "ffd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FixedFracDiff


def prices(rng, T, C, kind):
    """Price-like columns: a geometric walk from 20 .. 200, rounded to cents; `volume`: counts."""
    out = np.empty((T, C), dtype=np.float32)
    for c in range(C):
        if kind[c] == "volume":
            out[:, c] = np.round(np.exp(rng.normal(13.0, 0.6, T)))
        else:
            steps = rng.normal(2e-4, 0.012, T)
            out[:, c] = np.round(rng.uniform(20.0, 200.0) * np.exp(np.cumsum(steps)), 2)
    return out


def case(name, T, names, d, thres, seed, scaled=True):
    from sklearn.preprocessing import MinMaxScaler, StandardScaler
    FixedFracDiff = load_ffd()
    rng = np.random.default_rng(seed)
    raw = prices(rng, T + 1, len(names), names)
    close = torch.from_numpy(raw[:, names.index("close")])
    relatives = (close[1:] / close[:-1]).numpy()
    x = raw[1:]
    data = TensorDict({n: torch.from_numpy(x[:, i].copy()) for i, n in enumerate(names)})
    d_opt = {n: float(v) for n, v in zip(names, d) if n != "volume"}
    ffd = FixedFracDiff(data, thres, d_opt)
    out = ffd.fit_transform()
    mw = ffd.get_max_width()
    widths = np.zeros(len(names), dtype=np.int32)
    taps = []
    for i, f in enumerate(ffd.feats):
        if ffd.get_d_opt[f] > 0:
            widths[names.index(f)] = int(ffd.widths[i])
            taps.append(ffd.weights[i].flip(0).numpy().astype(np.float32))
    assert mw == widths.max()
    y = np.stack([out[n].numpy() for n in names], axis=1).astype(np.float32)
    assert y.shape == (T - mw, len(names))
    split = int(0.8 * len(y))
    rec = dict(raw=raw, relatives=relatives, names=np.array(names), d=np.asarray(d, dtype=np.float64),
               thres=np.float64(thres), widths=widths, max_width=np.int32(mw),
               taps=np.concatenate(taps) if taps else np.zeros(0, np.float32), ffd=y,
               split=np.int32(split), purge=np.int32(mw),
               source="zachramsey/pm-rl @ 2025-03-04 data/ffd.py FixedFracDiff (CPU), sklearn %s" %
                      __import__("sklearn").__version__)
    if scaled:
        for part, rows in (("train", y[:split]), ("test", y[split + mw:])):
            for tag, cls in (("minmax", MinMaxScaler), ("standard", StandardScaler)):
                cols = [torch.tensor(cls().fit_transform(torch.from_numpy(rows[:, c].copy()).reshape(-1, 1)).flatten())
                        for c in range(rows.shape[1])]                       # instrument.py:336
                rec[f"{part}_{tag}"] = torch.stack(cols, dim=1).numpy()     # float64: what sklearn returns for a tensor
    path = os.path.join(HERE, "ffd", f"ffd_{name}.npz")
    np.savez_compressed(path, **rec)
    print(f"{path}: T={T} widths={widths.tolist()} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    case("mixed_t600", 600, ["open", "high", "low", "close", "vwap", "volume"],
         [0.1, 0.3, 0.5, 0.7, 1.0, 0.0], 1e-3, seed=5)
    case("t6000", 6000, ["open", "high", "close"], [0.5, 0.3, 0.1], 1e-5, seed=6, scaled=False)
