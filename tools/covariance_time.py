#!/usr/bin/env python3
"""Posterior covariance at cfg2's shape (8192 chains x 100 dims) over G generations of resident history (default 1000: 6.5 GB): the
bpm_reduce_cov call (host-to-host around a call that ends in a device synchronise) and the whole param_est_cov-equivalent call (median of
5, warm), next to the project's own single full-window passes (bpm_reduce_moments, pass 0 of the quantile select) and, where
build_variants/mfma_f64_rate has been built (tools/micro/mfma_f64_rate.hip), the register-only FP64 matrix rate; then get_history() plus
np.cov on the same history, and whether the two agree within the derived bound 2 (n + 4) u sqrt(C_ii C_jj).
usage: covariance_time.py [G] [--out FILE] [--device-only]   (--device-only: no host copy / NumPy, for the kernel trace)"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _history_bench import PEAK_BW, Report, cfg2_engine, median_time, quantile_pass0_time  # noqa: E402
from bipymc_amd import _lib as L                      # noqa: E402
from bipymc_amd import covariance as CV               # noqa: E402



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
    n_burn, n, win_bytes, t = e.n_burn, e.n, e.win_bytes, e.target
    tiles = (d + 15) // 16
    flop = (n + 3) // 4 * (tiles * (tiles + 1) // 2) * 2048.0      # what the matrix cores execute: 16x16x4 per tile pair and 4 rows
    say("# posterior covariance at cfg2's shape: N = %d chains, d = %d, %d history rows (%.2f GB resident), window %d rows x %d; "
        "build %s" % (N, d, rows, rows * N * ld * 8 / 1e9, n, d, L.build_id(e.lib)))

    def run():
        return CV.compute(e.reduce_moments, e.reduce_cov, CV.single_process_allgather, n_burn, d)

    pc = run()                                     # warm-up
    center = pc.mean
    t_mom, _ = median_time(lambda: e.reduce_moments(n_burn))
    t_q0 = quantile_pass0_time(e, n_burn, d)
    t_cov, _ = median_time(lambda: e.reduce_cov(n_burn, center))
    t_call, pc = median_time(run)
    say("single full-window passes of this build, host-to-host: bpm_reduce_moments %.3f ms (%.2f TB/s); pass 0 of the quantile select "
        "%.3f ms (%.2f TB/s = %.3f of 8 TB/s)" % (t_mom * 1e3, win_bytes / t_mom / 1e12, t_q0 * 1e3, win_bytes / t_q0 / 1e12, win_bytes / t_q0 / PEAK_BW))
    say("bpm_reduce_cov host-to-host: %.3f ms; window read %.2f TB/s = %.3f of 8 TB/s; %.3g FP64 FLOP on the matrix cores = %.1f TFLOP/s; "
        "%.2f x the quantile pass" % (t_cov * 1e3, win_bytes / t_cov / 1e12, win_bytes / t_cov / PEAK_BW, flop, flop / t_cov / 1e12, t_cov / t_q0))
    say("param_est_cov() whole call (moments pass + covariance pass + host finish): %.3f ms; mean off-diagonal correlation %.4f (target rho %.2f; the window holds the burn-in)"
        % (t_call * 1e3, float(np.mean(pc.corr()[~np.eye(d, dtype=bool)])), t.rho))
    micro = os.path.join(ROOT, "build_variants", "mfma_f64_rate")
    if os.path.exists(micro):
        e.synchronize()
        out = subprocess.run([micro], stdout=subprocess.PIPE, timeout=120).stdout.decode()      # (a child process of its own)
        best = 0.0
        for ln in out.strip().splitlines():
            say(ln)
            if "TFLOP/s" in ln:
                best = max(best, float(ln.split(",")[-1].split()[0]))
        if best > 0:
            t_fl = flop / (best * 1e12)
            say("bounds: memory %.3f ms (the quantile pass), compute %.3f ms (%.3g FLOP at %.2f TFLOP/s); bpm_reduce_cov at %.3f ms is %.2f x the "
                "larger of the two, %.2f x their sum" % (t_q0 * 1e3, t_fl * 1e3, flop, best, t_cov * 1e3, t_cov / max(t_q0, t_fl), t_cov / (t_q0 + t_fl)))
    else:
        say("(build_variants/mfma_f64_rate not built: no register-only FP64 matrix rate)")
    if not a.device_only:
        t0 = time.perf_counter()
        H = e.get_history()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        want = np.cov(H.reshape(-1, d)[n_burn:], rowvar=False)
        t_np = time.perf_counter() - t0
        say("get_history(): %.2f s (%.2f GB to the host); np.cov on it: %.2f s; together %.2f s = %.0f x the device call"
            % (t_copy, H.nbytes / 1e9, t_np, t_copy + t_np, (t_copy + t_np) / t_call))
        sd = np.sqrt(np.diag(want))
        bound = 2.0 * (n + 4) * 2.0 ** -53 * np.outer(sd, sd)
        say("within 2 (n + 4) u sqrt(C_ii C_jj) of np.cov element by element: %s (largest error / bound %.2e); exactly symmetric: %s"
            % (bool(np.all(np.abs(pc.cov - want) <= bound)), float(np.max(np.abs(pc.cov - want) / bound)), bool(np.array_equal(pc.cov, pc.cov.T))))
    e.close()
    report.write(a.out)


if __name__ == "__main__":
    main()
