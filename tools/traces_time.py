#!/usr/bin/env python3
"""Per-generation trace summaries at cfg2's shape (8192 chains x 100 dims) over G generations of resident history (default 1000: 6.5 GB):
bpm_trace_bins with every = 1 (G + 1 short bins, one workgroup per bin and column tile) and with every = G + 1 (one long bin cut into
parts), host-to-host around calls that end in a device synchronise (median of 5, warm) -- these include the ln-like pass, the fold and
the copy of the per-bin records to the host; the time of tr_bins_kernel alone comes from `rocprofv3 --kernel-trace --stats` over
`traces_time.py --device-only` -- next to the project's own plain pass over the same window (bpm_hist_range), the bytes the pass reads
(rows x ld x 8) and the share of 8 TB/s they imply; then what a user of the parent commit does for the same picture: param_est(0)'s copy
(get_history + get_loglike_history) plus the NumPy reductions per generation, and whether the two agree.
usage: traces_time.py [G] [--out FILE] [--device-only]   (--device-only: no host copy / NumPy, for the kernel trace)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _history_bench import PEAK_BW, Report, cfg2_engine, median_time  # noqa: E402
from bipymc_amd import _lib as L                      # noqa: E402
from bipymc_amd import traces as TR                   # noqa: E402


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
    win_bytes = rows * N * ld * 8
    chains = [0, N // 2, N - 1, 17]
    say("# trace summaries at cfg2's shape: N = %d chains, d = %d, %d history rows (%.2f GB resident, all of them the window); build %s"
        % (N, d, rows, win_bytes / 1e9, L.build_id(e.lib)))

    def run(every):
        return TR.compute(e.trace_bins, e.trace_chains, TR.single_process_allgather, 0, N, rows, d, every=every, chains=chains)

    for every in (1, rows):                        # warm-up of every shape timed below
        run(every)
    e.hist_range(0)
    t_rng, _ = median_time(lambda: e.hist_range(0))
    say("plain pass over the window of this build, host-to-host: bpm_hist_range %.3f ms (%.2f TB/s = %.3f of 8 TB/s)"
        % (t_rng * 1e3, win_bytes / t_rng / 1e12, win_bytes / t_rng / PEAK_BW))
    for every in (1, rows):
        t_bins, _ = median_time(lambda: e.trace_bins(0, rows, every))
        t_call, pt = median_time(lambda: run(every))
        say("bpm_trace_bins, every = %d (%d bins), host-to-host: %.3f ms; it reads %d rows x %d x 8 = %.2f GB of states (+ %.3f GB of ln-likes): "
            "%.2f TB/s = %.3f of 8 TB/s; %.2f x the plain pass; param_est_trace() whole call with %d chains: %.3f ms"
            % (every, len(pt.gen), t_bins * 1e3, rows * N, ld, win_bytes / 1e9, rows * N * 8 / 1e9, win_bytes / t_bins / 1e12,
               win_bytes / t_bins / PEAK_BW, t_bins / t_rng, len(chains), t_call * 1e3))
    if not a.device_only:
        pt = run(1)
        t0 = time.perf_counter()
        H, LL = e.get_history(), e.get_loglike_history()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        mean, sd, mn, mx = H.mean(axis=1), H.std(axis=1), H.min(axis=1), H.max(axis=1)
        ll_mean, ll_max = LL.mean(axis=1), LL.max(axis=1)
        best = int(np.argmax(LL))
        t_np = time.perf_counter() - t0
        say("the parent commit's way: get_history() + get_loglike_history() %.2f s (%.2f GB to the host); np.mean / std / min / max per "
            "generation and the arg-max: %.2f s; together %.2f s = %.0f x param_est_trace(every = 1)"
            % (t_copy, (H.nbytes + LL.nbytes) / 1e9, t_np, t_copy + t_np, (t_copy + t_np) / median_time(lambda: run(1))[0]))
        say("min / max / best_row equal to NumPy: %s; largest |mean - np.mean| / sd: %.2e; largest |sd / np.std - 1|: %.2e; largest "
            "|ll_mean / np.mean - 1|: %.2e; ll_max equal: %s"
            % (bool(np.array_equal(pt.min, mn) and np.array_equal(pt.max, mx) and pt.best_row == best),
               float(np.max(np.abs(pt.mean - mean) / sd)), float(np.max(np.abs(pt.sd / sd - 1.0))),
               float(np.max(np.abs(pt.ll_mean / ll_mean - 1.0))), bool(np.array_equal(pt.ll_max, ll_max))))
    e.close()
    report.write(a.out)


if __name__ == "__main__":
    main()
