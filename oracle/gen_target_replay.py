#!/usr/bin/env python3
"""
ORACLE tooling (test infrastructure, not product code).

Records what the genuine reference's target objects (bipymc/utils/d100_gauss.py, dblgauss_rv.py, banana_rv.py) show the target
registry (bipymc_amd/utils/_target.py): every numeric attribute their constructors set, and ln_like at the points where the registry
checks its closed form against the callable.  tests/test_target_registry.py replays the recording, so the test needs neither the
reference nor its sources.

Usage:  python oracle/gen_target_replay.py --reference <checkout of wgurecky/bipymc> [--out tests/golden/reference_targets_replay.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

# label -> (module, class, constructor args); the test builds the shipped twin of each from the same label
OBJECTS = [("gauss100", "d100_gauss", "Gauss_100D", {}),
           ("gauss10_rho02", "d100_gauss", "Gauss_100D", {"rho": 0.2, "dim": 10}),
           ("bimodal", "dblgauss_rv", "BimodeGauss_2D", {}),
           ("banana_1_1", "banana_rv", "Banana_2D", {"mu1": 1, "mu2": 1}),
           ("banana", "banana_rv", "Banana_2D", {})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory holding the reference's bipymc package")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "reference_targets_replay.npz"))
    args = ap.parse_args()
    os.environ.setdefault("MPLBACKEND", "agg")
    sys.path.insert(0, os.path.abspath(args.reference))
    sys.dont_write_bytecode = True
    import importlib
    from bipymc_amd.utils import _target as T
    rec = {"labels": np.array([o[0] for o in OBJECTS])}
    for label, mod, cls, kw in OBJECTS:
        obj = getattr(importlib.import_module("bipymc.utils." + mod), cls)(**kw)
        dim = int(getattr(obj, "dim", 2))
        rec[label + ".class"] = np.array(type(obj).__name__)
        rec[label + ".module"] = np.array(type(obj).__module__)
        rec[label + ".dim"] = np.array(dim)
        for k, v in vars(obj).items():
            try:
                a = np.asarray(v, dtype=np.float64)
            except (TypeError, ValueError):
                continue                                   # (scipy's frozen distributions)
            rec["%s.attr.%s" % (label, k)] = a
        _, _, pts, _ = T._LOOKALIKES[cls][1](obj, dim)
        pts = np.array(pts, dtype=np.float64)
        with np.errstate(divide="ignore"):
            rec[label + ".points"] = pts
            rec[label + ".ln_like"] = np.array([float(np.asarray(obj.ln_like(p)).reshape(-1)[0]) for p in pts])
    np.savez_compressed(args.out, **rec)
    print("wrote %s (%d objects)" % (args.out, len(OBJECTS)))


if __name__ == "__main__":
    main()
