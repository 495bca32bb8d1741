#!/usr/bin/env python3
"""Rank-normalized diagnostics at cfg2's shape (8192 chains x 100 dims) over G generations of resident history (default 1000: 6.5 GB): the
whole convergence_diagnostics_rank() call, each of its four fills (bpm_rank_history: z, folded z, two indicators) and the diagnostics pass
over each, the classic convergence_diagnostics() over the same window, each timed host-to-host around calls that end in a device synchronise
(median of 3); an A/B of the sort's batch (BPM_RANK_BATCH_COLS); then get_history() plus the SciPy restatement (rankdata, ndtri, np.median,
np.quantile) on the first HOST_COLUMNS coordinates, its time scaled to all of them -- ranking 100 columns of 8 million values twice and
the FFT autocovariances of 4 x 100 columns take many minutes -- and the agreement.
usage: rank_diagnostics_time.py [G] [--out FILE] [--device-only]   (--device-only: no host copy / SciPy, for the kernel trace)
The record belongs in profiles/rank_diagnostics_cfg2.txt."""
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

HOST_COLUMNS = 4          # coordinates the host restatement ranks and computes R-hat / ESS of


def scipy_r_hat(H, prob):
    """the definitions of bipymc_amd/rank_diagnostics.py restated on a (G, N, d) host array -> (median, quantiles of all coordinates, seconds
    they took; r_hat_bulk, r_hat_tail and the four transformed arrays of the first HOST_COLUMNS coordinates)"""
    from scipy.special import ndtri
    from scipy.stats import rankdata
    G, N, d = H.shape
    n = G // 2
    W = np.concatenate([H[:n], H[G - n:]], axis=0)
    S = 2 * n * N
    flat = W.reshape(S, d)
    t0 = time.perf_counter()
    med, q = np.median(flat, axis=0), np.quantile(flat, prob, axis=0)
    t_q = time.perf_counter() - t0

    def z(col):
        return ndtri((rankdata(col, method="average") - 0.375) / (S + 0.25)).reshape(2 * n, N)

    def r_hat(x):             # x (2n, N): the half-chains side by side
        h = np.concatenate([x[:n], x[n:]], axis=1)
        Wv = h.var(axis=0, ddof=1).mean()
        return np.sqrt(((n - 1.0) / n * Wv + h.mean(axis=0).var(ddof=1)) / Wv)

    c = min(d, HOST_COLUMNS)
    rb, rt, keep = np.empty(c), np.empty(c), []
    for k in range(c):
        zb, zf = z(flat[:, k]), z(np.abs(flat[:, k] - med[k]))
        rb[k], rt[k] = r_hat(zb), r_hat(zf)
        keep.append((zb, zf, (W[:, :, k] <= q[0, k]).astype(float), (W[:, :, k] <= q[1, k]).astype(float)))
    return med, q, t_q, rb, rt, keep


def numpy_ess(x, n):
    """ESS of one transformed column x (2n, N) by the definitions of bipymc_amd/diagnostics.py (FFT autocovariances)"""
    h = np.concatenate([x[:n], x[n:]], axis=1)
    m = h.shape[1]
    xbar = h.mean(axis=0)
    Wv = h.var(axis=0, ddof=1).mean()
    varp = (n - 1.0) / n * Wv + xbar.var(ddof=1)
    f = np.fft.rfft(h - xbar, n=2 * n, axis=0)
    C = (np.fft.irfft(f * np.conj(f), n=2 * n, axis=0)[:n] / n).mean(axis=1)
    return m * n / D.geyer(1.0 - (Wv - C) / varp, n, m, n - 1)[0]


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
    say("# rank-normalized diagnostics at cfg2's shape: N = %d chains, d = %d, %d history rows (%.2f GB resident), S = %d values per "
        "coordinate (a sorted column: %.1f MB); build %s" % (N, d, rows, rows * N * ld * 8 / 1e9, S, S * 8 / 1e6, L.build_id(e.lib)))
    gather = D.single_process_allgather
    prob = RK.DEFAULT_PROB

    def whole():
        return RK.compute(e, gather, 0, rows, prob=prob)

    whole()                                                             # warm-up of every kernel
    t_rank, res = median_time(whole, reps=3)
    t_classic, cl = median_time(lambda: D.compute(e.diag_split_moments, e.diag_autocov, gather, 0, rows), reps=3)
    say("convergence_diagnostics_rank() whole call: %.1f ms; classic convergence_diagnostics() over the same window: %.1f ms (%.1f x)"
        % (t_rank * 1e3, t_classic * 1e3, t_rank / t_classic))
    say("  max r_hat %.5f (bulk %.5f, tail %.5f; classic %.5f); ESS bulk min / median %.0f / %.0f, tail %.0f / %.0f (classic %.0f / %.0f)"
        % (np.nanmax(res.r_hat), np.nanmax(res.r_hat_bulk), np.nanmax(res.r_hat_tail), np.nanmax(cl.r_hat), np.nanmin(res.ess_bulk),
           np.nanmedian(res.ess_bulk), np.nanmin(res.ess_tail), np.nanmedian(res.ess_tail), np.nanmin(cl.ess), np.nanmedian(cl.ess)))
    # the stages: each fill into one scratch handle, and the diagnostics pass over it
    pos = RK.positions_for(S, prob)
    dst, os_ = e.rank_history(0, rows, RK.KIND_Z, None, pos)
    try:
        win = 2 * n * N * ld * 8
        for name, kind, arg, pp in (("z (keys, sort, order statistics, scores)", RK.KIND_Z, None, pos),
                                    ("folded z (keys, sort, scores)", RK.KIND_Z_FOLDED, res.median, ()),
                                    ("indicator (no sort)", RK.KIND_INDICATOR, res.quantiles[0], ())):
            t_fill, _ = median_time(lambda: e.rank_history(0, rows, kind, arg, pp, dst), reps=3)
            t_diag, _ = median_time(lambda: D.compute(dst.diag_split_moments, dst.diag_autocov, gather, 0, 2 * n), reps=3)
            say("fill %-42s %.1f ms (the window read and written once is %.2f GB: %.2f TB/s = %.3f of 8 TB/s); diagnostics pass over it: %.1f ms"
                % (name + ":", t_fill * 1e3, 2 * win / 1e9, 2 * win / t_fill / 1e12, 2 * win / t_fill / PEAK_BW, t_diag * 1e3))
        for cols in (4, 16, 64):                                       # A/B: the batch of the segmented sort
            os.environ["BPM_RANK_BATCH_COLS"] = str(cols)
            e.rank_history(0, rows, RK.KIND_Z, None, (), dst)
            say("    BPM_RANK_BATCH_COLS=%d: z fill %.1f ms" % (cols, median_time(lambda: e.rank_history(0, rows, RK.KIND_Z, None, (), dst), reps=3)[0] * 1e3))
        del os.environ["BPM_RANK_BATCH_COLS"]
    finally:
        dst.close()
    if not a.device_only:
        t0 = time.perf_counter()
        H = e.get_history()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        med, q, t_q, rb, rt, keep = scipy_r_hat(H, prob)
        c = len(keep)
        t_r = (time.perf_counter() - t0 - t_q) * d / c
        t0 = time.perf_counter()
        ess = np.array([[numpy_ess(x, n) for x in col] for col in keep])
        t_e = (time.perf_counter() - t0) * d / c
        say("get_history(): %.2f s (%.2f GB to the host); SciPy restatement on it: np.median and np.quantile %.1f s; ranks, z scores and R-hat of "
            "%d of %d coordinates, scaled to all: %.1f s; their ESS, scaled to all: %.1f s; together %.1f s = %.0f x the device call"
            % (t_copy, H.nbytes / 1e9, t_q, c, d, t_r, t_e, t_copy + t_q + t_r + t_e, (t_copy + t_q + t_r + t_e) / t_rank))
        got = np.stack([res.ess_bulk, np.full(d, np.nan), res.ess_lower, res.ess_upper], axis=1)[:len(keep)]
        ess[:, 1] = np.nan                                                # (the folded array has an R-hat only)
        say("agreement with SciPy / NumPy: median and quantiles equal: %s; max rel diff r_hat_bulk %.2e, r_hat_tail %.2e, ESS (bulk, lower, upper "
            "of %d coordinates) %.2e" % (np.array_equal(res.median, med) and np.array_equal(res.quantiles, q), np.max(np.abs(res.r_hat_bulk[:c] / rb - 1)),
                                         np.max(np.abs(res.r_hat_tail[:c] / rt - 1)), c, np.nanmax(np.abs(got / ess - 1))))
    e.close()
    report.write(a.out)


if __name__ == "__main__":
    main()
