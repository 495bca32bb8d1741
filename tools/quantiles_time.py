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
from _history_bench import PEAK_BW, Report, cfg2_engine, median_time  # noqa: E402
from bipymc_amd import _lib as L                      # noqa: E402
from bipymc_amd import quantiles as Q                 # noqa: E402



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("G", nargs="?", type=int, default=1000)
    ap.add_argument("--q", default="0.05,0.5,0.95")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    q = [float(x) for x in a.q.split(",")]
    report = Report()
    say = report.say
    e = cfg2_engine(a.G)
    N, d, rows, ld = e.N, e.d, e.rows, e.ld
    n_burn, win_bytes = e.n_burn, e.win_bytes
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
    report.write(a.out)


if __name__ == "__main__":
    main()
