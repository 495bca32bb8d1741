#!/usr/bin/env python3
"""Posterior quantiles at cfg2's shape (8192 chains x 100 dims) over G generations of resident history (default 1000: 6.5 GB): every
histogram pass of the radix select (host-to-host around a call that ends in a device synchronise) and the whole param_est_quantiles-
equivalent call (median of 5); then get_history() plus np.quantile on the same history, and whether the two agree value for value.
usage: quantiles_time.py [G] [--q 0.05,0.5,0.95] [--out FILE] [--device-only]   (--device-only: no host copy / NumPy, for the kernel trace)"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bipymc_amd import _lib as L                      # noqa: E402
from bipymc_amd import quantiles as Q                 # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("G", nargs="?", type=int, default=1000)
    ap.add_argument("--q", default="0.05,0.5,0.95")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    q = [float(x) for x in a.q.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = 8192
    t = d100_gauss.Gauss_100D()
    tid, tp, d = t._bpm_target_spec()
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=1, burnin_gen=100, n_cr_gen=20)
    e.set_state(np.random.RandomState(0).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0))
    e.reserve_history(a.G + 1)
    e.begin_run()
    e.step(a.G)
    e.synchronize()
    rows = e.history_rows()
    ld = d + (d & 1)
    n_burn = N                                     # the initial state left out
    win_bytes = (rows * N - n_burn) * ld * 8
    say("# posterior quantiles at cfg2's shape: N = %d chains, d = %d, %d history rows (%.2f GB resident), window %d rows x %d, q = %s; "
        "build %s" % (N, d, rows, rows * N * ld * 8 / 1e9, rows * N - n_burn, d, a.q, L.build_id(e.lib)))

    def run():
        return Q.compute(e.quantile_begin, e.quantile_histogram, Q.single_process_allgather, n_burn, q, dim=d)

    run()                                          # warm-up
    passes = []

    def timed_hist(pk, pv, bits):
        t0 = time.perf_counter()
        out = e.quantile_histogram(pk, pv, bits)
        passes.append((bits, len(pk), time.perf_counter() - t0))
        return out

    for _ in range(5):
        Q.compute(e.quantile_begin, timed_hist, Q.single_process_allgather, n_burn, q, dim=d)
    n_pass = Q.PASSES
    for p in range(n_pass):
        ts = [x[2] for x in passes[p::n_pass]]
        tp_ = float(np.median(ts))
        say("pass %d (prefix %2d bits, %4d histograms, bpm_quantile_histogram host-to-host): %.3f ms, window read %.2f TB/s = %.3f of 8 TB/s"
            % (p, passes[p][0], passes[p][1], tp_ * 1e3, win_bytes / tp_ / 1e12, win_bytes / tp_ / PEAK_BW))
    t_call, res = median_time(run)
    say("param_est_quantiles() whole call: %.2f ms; %d full-window passes (%.2f GB each); median over coordinates of the %s quantiles: %s"
        % (t_call * 1e3, n_pass, win_bytes / 1e9, a.q, np.array2string(np.median(res, axis=1), precision=4)))
    if not a.device_only:
        t0 = time.perf_counter()
        H = e.get_history()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        want = np.quantile(H.reshape(-1, d)[n_burn:], q, axis=0)
        t_np = time.perf_counter() - t0
        say("get_history(): %.2f s (%.2f GB to the host); np.quantile on it: %.2f s; together %.2f s = %.0f x the device call"
            % (t_copy, H.nbytes / 1e9, t_np, t_copy + t_np, (t_copy + t_np) / t_call))
        say("equal to np.quantile value for value: %s" % bool(np.array_equal(res, want, equal_nan=True)))
    e.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
