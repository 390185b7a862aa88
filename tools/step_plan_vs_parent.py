"""The step's kernel choice of this build against another build's library (the parent
commit's), handle by handle on the GPU: for shapes one env either side of every byte threshold
of the plan, both libraries create a handle, and pmenv_step_path under AUTO and under each
forced path, with pmenv_create's and pmenv_set_step_path's return codes, must be equal.

    python tools/step_plan_vs_parent.py --parent-lib PATH [--commit SHA] --out profiles/step_plan_vs_parent.json

Each handle's device memory (the state, the snapshot, the relay words) stays under 0.5 GB; the
windows themselves are the caller's and are never allocated here."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pm-rl_amd"))

import torch  # noqa: E402,F401  (first: both libraries bind to the HIP runtime torch loaded)
from pmenv import _abi  # noqa: E402

MIB = 1 << 20
THRESHOLDS = [m * MIB for m in (2, 16, 24, 48, 100, 128, 192, 256, 1024)]
# (N, W, F, commission): the flat / relay / one-workgroup bands at four fills, wide envs in
# both packed forms, the generic stream over the register and the tiny step, a non-granular window
FAMILIES = [(30, 50, 5, 0.0), (8, 50, 5, 0.0), (16, 50, 5, 0.0025), (64, 50, 5, 0.0), (100, 50, 5, 0.0),
            (500, 50, 5, 0.0), (30, 50, 8, 0.0), (5, 50, 8, 0.0), (33, 13, 5, 0.0)]
SMALL = [(1, 5, 50, 5, 0.0), (64, 30, 50, 5, 0.0), (41, 7, 6, 3, 0.0), (128, 30, 50, 8, 0.0), (256, 65, 50, 5, 0.0),
         (5, 30, 50, 5, 0.0), (5, 1, 4, 5, 0.0), (5, 4, 20, 5, 0.0), (8, 30, 50, 17, 0.0), (16, 100, 50, 8, 0.0),
         (7, 513, 3, 5, 0.0), (4, 30, 4000, 5, 0.0), (4, 6000, 2, 5, 0.0)]


def load(path):
    lib = ctypes.CDLL(path)
    for name, res, args in _abi.SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def shapes():
    out = list(SMALL)
    for N, W, F, cm in FAMILIES:
        env_bytes = N * W * F * 4
        for t in THRESHOLDS:
            out += [(t // env_bytes, N, W, F, cm), (t // env_bytes + 1, N, W, F, cm)]
    return out


def answers(lib, B, N, W, F, cm):
    """[create's rc, AUTO's path, then (rc, path) per forced path] from one handle of lib."""
    c = _abi.PmenvCfg()
    lib.pmenv_cfg_default(ctypes.byref(c), B, N, W, F)
    c.commission = cm
    h = ctypes.c_void_p()
    rc = lib.pmenv_create(ctypes.byref(c), 0, ctypes.byref(h))
    if rc != 0:
        return [rc]
    out = [rc, lib.pmenv_step_path(h).decode()]
    for path in sorted(_abi.STEP_PATHS.values()):
        out.append([lib.pmenv_set_step_path(h, path), lib.pmenv_step_path(h).decode()])
    lib.pmenv_destroy(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--commit", default=None, help="the commit the parent library was built from (recorded)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    this, parent = _abi.load(), load(a.parent_lib)
    compared, mismatches = [], []
    for s in shapes():
        x, y = answers(this, *s), answers(parent, *s)
        compared.append({"shape": list(s), "create_rc": x[0], "auto": x[1] if len(x) > 1 else None})
        if x != y:
            mismatches.append({"shape": list(s), "this": x, "parent": y})
        torch.cuda.synchronize()
    res = {"parent_commit": a.commit, "device": torch.cuda.get_device_name(0), "shapes_compared": len(compared),
           "paths_per_shape": ["auto"] + sorted(_abi.STEP_PATHS, key=_abi.STEP_PATHS.get),
           "mismatches": mismatches, "compared": compared}
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: res[k] for k in ("parent_commit", "shapes_compared", "mismatches")}))
    return 1 if mismatches else 0


if __name__ == "__main__":
    sys.exit(main())
