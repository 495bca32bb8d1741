"""What tools/{diagnostics,quantiles,covariance,histograms}_time.py share: the cfg2-shaped engine with G generations of resident history,
the median timer, the report that prints and keeps its lines for --out, and the plain pass over the window the statistics are compared with."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from bipymc_amd import _lib as L                      # noqa: E402
from bipymc_amd.engine import HipEngine               # noqa: E402
from bipymc_amd.utils import d100_gauss               # noqa: E402

PEAK_BW = 8.0e12          # HBM3E spec (MI355X_MICROARCH.md)


def median_time(fn, reps=5):
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


class Report(object):
    """say(line) prints it at once; write(path) leaves every line said in a file (--out; None: nothing)"""

    def __init__(self):
        self.lines = []

    def say(self, s):
        print(s, flush=True)
        self.lines.append(s)

    def write(self, path):
        if path:
            with open(path, "w") as f:
                f.write("\n".join(self.lines) + "\n")


def cfg2_engine(G):
    """cfg2's shape: DREAM, 8192 chains x the 100-D Gaussian, state set, history reserved, G generations stepped, synchronised.
    -> the engine, with N, d, target (the Gauss_100D), rows (history rows), ld (row pitch), n_burn (= N: the initial state left out),
    n (rows of the window) and win_bytes set on it"""
    N = 8192
    t = d100_gauss.Gauss_100D()
    tid, tp, d = t._bpm_target_spec()
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=1, burnin_gen=100, n_cr_gen=20)
    e.set_state(np.random.RandomState(0).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0))
    e.reserve_history(G + 1)
    e.begin_run()
    e.step(G)
    e.synchronize()
    e.N, e.d, e.target = N, d, t
    e.rows = e.history_rows()
    e.ld = d + (d & 1)
    e.n_burn = N
    e.n = e.rows * N - e.n_burn
    e.win_bytes = e.n * e.ld * 8
    return e


def quantile_pass0_time(e, n_burn, d):
    """pass 0 of the quantile select (one 256-bin histogram per coordinate): the project's own plain pass over the window, host-to-host"""
    e.quantile_begin(n_burn)
    pk, pv = np.arange(d, dtype=np.int32), np.zeros(d, dtype=np.uint64)
    e.quantile_histogram(pk, pv, 0)
    return median_time(lambda: e.quantile_histogram(pk, pv, 0))[0]
