#!/usr/bin/env python3
"""Convergence diagnostics at cfg2's shape (8192 chains x 100 dims) over G generations of resident history (default 1000: 6.5 GB): the
split-moments pass, every autocovariance lag block and the whole convergence_diagnostics() call, each timed host-to-host around a call that
ends in a device synchronise (median of 5); then get_history() plus a NumPy restatement on the same history, and the agreement of the two.
usage: diagnostics_time.py [G] [--out FILE] [--device-only]   (--device-only: no host copy / NumPy, for the kernel trace)"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _history_bench import PEAK_BW, Report, cfg2_engine, median_time  # noqa: E402
from bipymc_amd import _lib as L                      # noqa: E402
from bipymc_amd import diagnostics as D               # noqa: E402

PEAK_FP64 = 78.6e12       # FP64 vector spec of the MI355X (FMA = 2 FLOP)


def numpy_diagnostics(H, max_lag):
    """the definitions of bipymc_amd/diagnostics.py restated in NumPy on a (G, N, d) host array (FFT autocovariances)"""
    G = H.shape[0]
    n = G // 2
    halves = np.concatenate([H[:n], H[G - n:]], axis=1)
    m, d = halves.shape[1], halves.shape[2]
    xbar = halves.mean(axis=0)
    W = halves.var(axis=0, ddof=1).mean(axis=0)
    varp = (n - 1.0) / n * W + xbar.var(axis=0, ddof=1)
    r_hat = np.sqrt(varp / W)
    ess = np.empty(d)
    for k in range(d):
        y = halves[:, :, k] - xbar[:, k]
        f = np.fft.rfft(y, n=2 * n, axis=0)
        C = (np.fft.irfft(f * np.conj(f), n=2 * n, axis=0)[:n] / n).mean(axis=1)
        rho = 1.0 - (W[k] - C) / varp[k]
        tau, _l, _c = D.geyer(rho, n, m, min(max_lag, n - 1) if max_lag else n - 1)
        ess[k] = m * n / tau
    return r_hat, ess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("G", nargs="?", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    report = Report()
    say = report.say
    e = cfg2_engine(a.G)
    N, d, rows, ld = e.N, e.d, e.rows, e.ld
    say("# convergence diagnostics at cfg2's shape: N = %d chains, d = %d, %d history rows (%.2f GB resident); build %s"
        % (N, d, rows, rows * N * ld * 8 / 1e9, L.build_id(e.lib)))
    # warm-up of every kernel
    D.compute(e.diag_split_moments, e.diag_autocov, D.single_process_allgather, 0, rows)
    n = rows // 2
    t_split, _ = median_time(lambda: e.diag_split_moments(0, rows))
    nbytes = 2 * n * N * ld * 8
    say("split-moments pass (bpm_diag_split_moments, host-to-host incl. the across-half-chain kernel and a sync): %.3f ms for %.2f GB "
        "-> %.2f TB/s = %.3f of 8 TB/s" % (t_split * 1e3, nbytes / 1e9, nbytes / t_split / 1e12, nbytes / t_split / PEAK_BW))
    blocks = []
    for t0 in (0, 16, 32, 48, 64):
        tb, _ = median_time(lambda: e.diag_autocov(t0, D.LAG_BLOCK))
        fma = 2 * N * d * sum(max(0, n - tt) for tt in range(t0, t0 + D.LAG_BLOCK))
        blocks.append(tb)
        say("autocovariance lags [%d, %d) (bpm_diag_autocov, host-to-host): %.3f ms, %.3e FMA -> %.2f TFLOP/s FP64 = %.3f of 78.6; "
            "window read %.2f TB/s" % (t0, t0 + D.LAG_BLOCK, tb * 1e3, fma, 2 * fma / tb / 1e12, 2 * fma / tb / PEAK_FP64,
                                       nbytes / tb / 1e12))
    t_call, res = median_time(lambda: D.compute(e.diag_split_moments, e.diag_autocov, D.single_process_allgather, 0, rows), reps=3)
    say("convergence_diagnostics() whole call: %.2f ms; max r_hat %.5f, ESS min / median %.0f / %.0f, lags used max %d"
        % (t_call * 1e3, np.nanmax(res.r_hat), np.nanmin(res.ess), np.nanmedian(res.ess), res.lags_used.max()))
    if not a.device_only:
        t0 = time.perf_counter()
        H = e.get_history()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        r_np, ess_np = numpy_diagnostics(H, None)
        t_np = time.perf_counter() - t0
        say("get_history(): %.2f s (%.2f GB to the host); NumPy restatement on it: %.2f s; together %.2f s = %.0f x the device call"
            % (t_copy, H.nbytes / 1e9, t_np, t_copy + t_np, (t_copy + t_np) / t_call))
        say("agreement with NumPy: max rel diff r_hat %.2e, ESS %.2e"
            % (np.max(np.abs(res.r_hat / r_np - 1)), np.max(np.abs(res.ess / ess_np - 1))))
    e.close()
    report.write(a.out)


if __name__ == "__main__":
    main()
