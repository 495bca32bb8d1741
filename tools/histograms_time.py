#!/usr/bin/env python3
"""Posterior histograms at cfg2's shape (8192 chains x 100 dims) over G generations of resident history (default 1000: 6.5 GB): the range
pass, the marginal pass at 20 bins, the pair pass for every pair of 8 coordinates (28 pairs) at 20 x 20 bins and the whole
param_est_hist-equivalent call (host-to-host around calls that end in a device synchronise; median of 5, warm), next to the project's own
plain pass over the same window (pass 0 of the quantile select), measured in the same run; then get_history() plus np.histogram and
np.histogram2d on the same history, and whether the counts agree.
usage: histograms_time.py [G] [--out FILE] [--device-only]   (--device-only: no host copy / NumPy, for the kernel trace)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _history_bench import PEAK_BW, Report, cfg2_engine, median_time, quantile_pass0_time  # noqa: E402
from bipymc_amd import _lib as L                      # noqa: E402
from bipymc_amd import histograms as HS               # noqa: E402



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
    n_burn, n, win_bytes = e.n_burn, e.n, e.win_bytes
    pair_dims = list(range(8))
    say("# posterior histograms at cfg2's shape: N = %d chains, d = %d, %d history rows (%.2f GB resident), window %d rows x %d; "
        "build %s" % (N, d, rows, rows * N * ld * 8 / 1e9, n, d, L.build_id(e.lib)))

    def run():
        return HS.compute(e.hist_range, e.hist_marginals, e.hist_pairs, HS.single_process_allgather, n_burn, d, pairs=None)

    def run_pairs():
        return HS.compute(e.hist_range, e.hist_marginals, e.hist_pairs, HS.single_process_allgather, n_burn, d, dims=pair_dims, pairs="all")

    ph = run()                                     # warm-up
    pp = run_pairs()
    t_q0 = quantile_pass0_time(e, n_burn, d)
    t_rng, _ = median_time(lambda: e.hist_range(n_burn))
    t_mar, _ = median_time(lambda: e.hist_marginals(ph.dims, ph.edges))
    pos = {int(k): j for j, k in enumerate(pp.dims)}
    pa = [pos[int(x)] for x in pp.pairs[:, 0]]
    pb = [pos[int(x)] for x in pp.pairs[:, 1]]
    t_pair, _ = median_time(lambda: e.hist_pairs(pp.dims, pp.edges2d, pa, pb))
    t_call, ph = median_time(run)
    t_callp, pp = median_time(run_pairs)
    say("plain pass over the window of this build, host-to-host: pass 0 of the quantile select %.3f ms (%.2f TB/s = %.3f of 8 TB/s)"
        % (t_q0 * 1e3, win_bytes / t_q0 / 1e12, win_bytes / t_q0 / PEAK_BW))
    say("bpm_hist_range host-to-host: %.3f ms (%.2f TB/s); %.2f x the quantile pass" % (t_rng * 1e3, win_bytes / t_rng / 1e12, t_rng / t_q0))
    say("bpm_hist_marginals, %d coordinates x %d bins: %.3f ms (%.2f TB/s); %.2f x the quantile pass"
        % (d, ph.counts.shape[1], t_mar * 1e3, win_bytes / t_mar / 1e12, t_mar / t_q0))
    say("bpm_hist_pairs, %d pairs of %d coordinates x %d x %d bins: %.3f ms; %.2f x the quantile pass (it reads %d of the %d columns)"
        % (len(pp.pairs), len(pair_dims), pp.counts2d.shape[1], pp.counts2d.shape[2], t_pair * 1e3, t_pair / t_q0, len(pair_dims), ld))
    say("param_est_hist() whole call, all marginals (range pass + marginal pass + host): %.3f ms; with dims = 0..7 and pairs = \"all\" "
        "(range + marginals of 8 + 28 pairs): %.3f ms" % (t_call * 1e3, t_callp * 1e3))
    peak = ph.counts.max(axis=1) / ph.n
    say("share of the rows in the fullest bin of a coordinate: median %.3f, largest %.3f" % (float(np.median(peak)), float(peak.max())))
    if not a.device_only:
        t0 = time.perf_counter()
        H = e.get_history()
        t_copy = time.perf_counter() - t0
        W = H.reshape(-1, d)[n_burn:]
        t0 = time.perf_counter()
        ok1 = all(np.array_equal(np.histogram(W[:, k], 20)[0], ph.counts[k]) for k in range(d))
        t_np1 = time.perf_counter() - t0
        t0 = time.perf_counter()
        ok2 = all(np.array_equal(np.histogram2d(W[:, x], W[:, y], 20)[0], pp.counts2d[p]) for p, (x, y) in enumerate(pp.pairs))
        t_np2 = time.perf_counter() - t0
        say("get_history(): %.2f s (%.2f GB to the host); np.histogram of %d columns: %.2f s; np.histogram2d of %d pairs: %.2f s; together "
            "%.2f s = %.0f x the two device calls (%.3f ms)" % (t_copy, H.nbytes / 1e9, d, t_np1, len(pp.pairs), t_np2, t_copy + t_np1 + t_np2,
                                                                (t_copy + t_np1 + t_np2) / (t_call + t_callp), (t_call + t_callp) * 1e3))
        say("counts equal to np.histogram: %s; to np.histogram2d: %s; every marginal row sums to n: %s"
            % (ok1, ok2, bool(np.all(ph.counts.sum(axis=1) == ph.n))))
    e.close()
    report.write(a.out)


if __name__ == "__main__":
    main()
