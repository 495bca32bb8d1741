#!/usr/bin/env python3
"""The posterior summary at cfg2's shape (8192 chains x 100 dims) over G generations of resident history (default 1000: 6.5 GB): the whole
posterior_summary() call, host-to-host; the bpm_hdi call alone with one and with eight probabilities -- a scan of a sorted column reads
col[i] and col[i + m] for i < S - m, 16 (S - m) bytes, so the difference of the two calls is the scan (rk_hdi_kernel + rk_hdi_final_kernel)
over the difference of their bytes, given as a fraction of 8 TB/s (the kernel's own time: a rocprofv3 --kernel-trace --stats run of its own
over --device-only) -- and the squared-deviation fill; convergence_diagnostics_rank() on the same build for scale; then get_history() plus the NumPy / SciPy
restatement on the first HOST_COLUMNS coordinates, its time scaled to all of them (np.sort and the widths, mean, sd, the FFT autocovariances
of x and of (x - mean)^2) and the agreement.  Each figure is the median of 3 around calls that end in a device synchronise.
usage: summary_time.py [G] [--out FILE] [--device-only]   (--device-only: no host copy / NumPy, for a kernel trace)
The record belongs in profiles/summary_cfg2.txt."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _history_bench import PEAK_BW, Report, cfg2_engine, median_time  # noqa: E402
from bipymc_amd import _lib as L                      # noqa: E402
from bipymc_amd import diagnostics as D               # noqa: E402
from bipymc_amd import rank_diagnostics as RK         # noqa: E402
from bipymc_amd import summary as SM                  # noqa: E402
from rank_diagnostics_time import numpy_ess           # noqa: E402

HOST_COLUMNS = 4          # coordinates the host restatement computes the two ESS of
HDI_PROB = 0.94


def numpy_hdi(flat, p):
    """summary.py's definition on a (S, d) host array -> (lo, hi)"""
    S = len(flat)
    m = SM.hdi_offset(p, S)
    s = np.sort(flat + 0.0, axis=0)
    w = s[m:] - s[:S - m]
    i = np.argmin(w, axis=0)
    k = np.arange(flat.shape[1])
    return s[i, k], s[i + m, k]


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
    n, S = RK.split_size(0, rows, N)
    say("# posterior summary at cfg2's shape: N = %d chains, d = %d, %d history rows (%.2f GB resident), S = %d values per coordinate (a "
        "sorted column: %.1f MB); build %s" % (N, d, rows, rows * N * ld * 8 / 1e9, S, S * 8 / 1e6, L.build_id(e.lib)))
    gather = D.single_process_allgather

    def whole():
        return SM.compute(e, gather, 0, rows, hdi_prob=HDI_PROB)

    whole()                                                             # warm-up of every kernel
    t_sum, res = median_time(whole, reps=3)
    t_rank, _ = median_time(lambda: RK.compute(e, gather, 0, rows), reps=3)
    t_classic, _ = median_time(lambda: D.compute(e.diag_split_moments, e.diag_autocov, gather, 0, rows), reps=3)
    say("posterior_summary() whole call: %.1f ms; convergence_diagnostics_rank() over the same window: %.1f ms (%.2f x); classic "
        "convergence_diagnostics(): %.1f ms" % (t_sum * 1e3, t_rank * 1e3, t_sum / t_rank, t_classic * 1e3))
    say("  max r_hat %.5f; ESS mean min / median %.0f / %.0f, sd %.0f / %.0f; largest mcse_mean / sd %.4f, mcse_sd / sd %.4f"
        % (np.nanmax(res.r_hat), np.nanmin(res.ess_mean), np.nanmedian(res.ess_mean), np.nanmin(res.ess_sd), np.nanmedian(res.ess_sd),
           np.nanmax(res.mcse_mean / res.sd), np.nanmax(res.mcse_sd / res.sd)))
    p8 = np.linspace(0.5, 0.99, 8)

    def scan_bytes(probs):
        return 16.0 * d * sum(S - SM.hdi_offset(p, S) for p in probs)

    t_h1, _ = median_time(lambda: e.hdi(SM.WINDOW_SPLIT_ROWS, 0, rows, [HDI_PROB]), reps=3)
    t_h8, _ = median_time(lambda: e.hdi(SM.WINDOW_SPLIT_ROWS, 0, rows, p8), reps=3)
    scan, more = max(t_h8 - t_h1, 1e-9), scan_bytes(p8) - scan_bytes([HDI_PROB])
    say("bpm_hdi alone (keys, sort, scan): %.1f ms with p = %.2f (the scan reads %.2f GB), %.1f ms with 8 probabilities from 0.5 to 0.99 (%.2f GB); "
        "the difference: %.2f ms for %.2f GB = %.2f TB/s = %.3f of 8 TB/s"
        % (t_h1 * 1e3, HDI_PROB, scan_bytes([HDI_PROB]) / 1e9, t_h8 * 1e3, scan_bytes(p8) / 1e9, scan * 1e3, more / 1e9, more / scan / 1e12,
           more / scan / PEAK_BW))
    t_pe, _ = median_time(lambda: e.hdi(SM.WINDOW_PARAM_EST, N, 0, [HDI_PROB]), reps=3)
    say("  over param_est's window (n_burn = %d, %d values per coordinate): %.1f ms" % (N, rows * N - N, t_pe * 1e3))
    dst, _ = e.rank_history(0, rows, RK.KIND_SQDEV, res.mean)
    try:
        win = 2 * n * N * ld * 8
        t_fill, _ = median_time(lambda: e.rank_history(0, rows, RK.KIND_SQDEV, res.mean, (), dst), reps=3)
        t_diag, _ = median_time(lambda: D.compute(dst.diag_split_moments, dst.diag_autocov, gather, 0, 2 * n), reps=3)
        say("squared-deviation fill (no sort): %.1f ms (the window read and written once is %.2f GB: %.2f TB/s = %.3f of 8 TB/s); diagnostics "
            "pass over it: %.1f ms" % (t_fill * 1e3, 2 * win / 1e9, 2 * win / t_fill / 1e12, 2 * win / t_fill / PEAK_BW, t_diag * 1e3))
    finally:
        dst.close()
    if not a.device_only:
        t0 = time.perf_counter()
        H = e.get_history()
        t_copy = time.perf_counter() - t0
        W = np.concatenate([H[:n], H[rows - n:]], axis=0)
        flat = W.reshape(S, d)
        t0 = time.perf_counter()
        c = min(d, HOST_COLUMNS)
        part = np.ascontiguousarray(flat[:, :c])
        lo, hi = numpy_hdi(part, HDI_PROB)
        mean, sd = part.mean(axis=0), part.std(axis=0, ddof=1)
        t_hdi = (time.perf_counter() - t0) * d / c
        t0 = time.perf_counter()
        ess = np.array([[numpy_ess(W[:, :, k], n), numpy_ess((W[:, :, k] - mean[k]) ** 2, n)] for k in range(c)])
        t_e = (time.perf_counter() - t0) * d / c
        host = t_copy + t_hdi + t_e
        say("get_history(): %.2f s (%.2f GB to the host); NumPy restatement on %d of %d coordinates, scaled to all: sort, widths, mean and sd %.1f s; the ESS "
            "of x and of (x - mean)^2 %.1f s; together %.1f s -- without the rank diagnostics, which "
            "tools/rank_diagnostics_time.py times -- = %.0f x the device call" % (t_copy, H.nbytes / 1e9, c, d, t_hdi, t_e, host, host / t_sum))
        say("agreement with NumPy on those coordinates: hdi equal: %s; max rel diff mean %.2e, sd %.2e, ESS (mean, sd) %.2e"
            % (np.array_equal(res.hdi_lo[:c], lo) and np.array_equal(res.hdi_hi[:c], hi), np.max(np.abs(res.mean[:c] / mean - 1)),
               np.max(np.abs(res.sd[:c] / sd - 1)), np.max(np.abs(np.stack([res.ess_mean[:c], res.ess_sd[:c]], axis=1) / ess - 1))))
    e.close()
    report.write(a.out)


if __name__ == "__main__":
    main()
