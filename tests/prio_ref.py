"""A numpy f64 restatement of the priority tree (include/pmenv.h, "prioritized sampling";
Schaul et al. 2016, proportional variant) for tests/test_gpu_prio.py, and a reader of the
device buffer's levels."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def read_tree(tree, leaves):
    """(maximum, [level 0 = the f32 leaves, level 1.. = f64 nodes]) of a device tree buffer."""
    from pmenv.replay import prio_layout
    raw = tree.cpu().numpy()
    lay = prio_layout(leaves)
    assert raw.nbytes == lay["bytes"]
    levels = [raw[off:off + n * np.dtype(dt).itemsize].view(dt).copy() for off, n, dt in lay["levels"]]
    return raw[:4].view(np.float32)[0], levels


def node_sums(children):
    """The f64 sums of runs of 64 children (the last run may be short)."""
    c = np.asarray(children, dtype=np.float64)
    pad = np.zeros((len(c) + 63) // 64 * 64)
    pad[:len(c)] = c
    return pad.reshape(-1, 64).sum(axis=1)


def check_levels(levels, rel=1e-12):
    """Every internal node is the f64 sum of its children to `rel`; the level sizes are
    ceil(n / 64) down to a top level of at most 64 nodes."""
    assert len(levels) >= 2 and len(levels[-1]) <= 64
    for k in range(1, len(levels)):
        want = node_sums(levels[k - 1])
        assert len(levels[k]) == len(want) and (k == len(levels) - 1 or len(levels[k]) > 64)
        assert np.all(np.abs(levels[k] - want) <= rel * want), f"level {k}"


def ancestors(leaf_idx, n_levels):
    """For each internal level k, the node indices that have one of the leaves below them."""
    idx = np.unique(np.asarray(leaf_idx, dtype=np.int64))
    out = []
    for _ in range(n_levels):
        idx = np.unique(idx >> 6)
        out.append(idx)
    return out


def priority(td, alpha, eps, cur_max):
    """max((|td| + eps)^alpha, FLT_MIN) in f64, rounded once to f32; non-finite td: cur_max."""
    td = np.asarray(td, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.power(np.abs(td).astype(np.float64) + eps, alpha)
        v = np.clip(v, FLT_MIN, FLT_MAX).astype(np.float32)
    return np.where(np.isfinite(td), v, np.float32(cur_max)).astype(np.float32)


def weights(p, beta):
    """(p_j / min_k p_k)^(-beta) in f64, rounded once to f32."""
    p = np.asarray(p, dtype=np.float64)
    return np.power(p / p.min(), -beta).astype(np.float32)
