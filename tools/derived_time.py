#!/usr/bin/env python3
"""Derived-quantity summaries at cfg2's shape (8192 chains x 100 dims) over G generations of resident history (default 1000: 6.5 GB):
param_est_fn's whole call (bpm_set_device_function with the module already loaded + bpm_derive + the host merge), host-to-host, median of 5,
warm, for n_out = 1 (a ratio of two parameters) and n_out = 64 (a line on 64 abscissae), against
  (a) what a user of the parent commit does: get_history() + get_loglike_history() and the NumPy statement with np.mean / np.std / np.min /
      np.max over its values, and
  (b) bpm_reduce_moments over the same window in the same run: the project's plain single-read pass,
with the bytes the pass reads (rows x ld x 8) and the share of 8 TB/s they imply, the one-off compilation time, and whether device and
NumPy agree.
Then the derived history (sampler.derived_history: bpm_derive_history, the fill kernel bpm_derive_fill) for the same two functions over the
whole resident history: the build host-to-host, the bytes it reads and writes (rows x ld x 8 + rows x ldd x 8) and the share of 8 TB/s they
imply, dh.param_est_quantiles at 5 / 50 / 95 %, next to bpm_derive over the same rows in the same run and -- unless --device-only -- the
route of the parent commit, param_est_fn(values=True) + np.quantile.  The fill kernel's own time comes from a run of
`rocprofv3 --kernel-trace --stats -- python tools/derived_time.py --device-only` (kernel bpm_derive_fill); the record goes to
profiles/derived_history_cfg2.txt.
usage: derived_time.py [G] [--out FILE] [--device-only]   (--device-only: no host copy / NumPy)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _history_bench import PEAK_BW, Report, cfg2_engine, median_time  # noqa: E402
from bipymc_amd import HipFunction                    # noqa: E402
from bipymc_amd import _lib as L                      # noqa: E402
from bipymc_amd import derived as DV                  # noqa: E402

RATIO = HipFunction("""
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) { out[0] = x[2] / x[1]; }""", n_out=1,
                    python_fn=lambda X, ll, p: (X[:, 2] / X[:, 1])[:, None])
LINE = HipFunction("""
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    for (int k = 0; k < 64; ++k) out[k] = x[0] + x[1] * p[k];
}""", n_out=64, params=np.linspace(0.0, 1.0, 64), python_fn=lambda X, ll, p: X[:, :1] + X[:, 1:2] * p[None, :])


def derived_history_section(e, say, device_only):
    from bipymc_amd._history_stats import HistoryStatistics

    class Over(HistoryStatistics):
        n_chains = e.N
        _stats_allgather = staticmethod(DV.single_process_allgather)

        def _stats_engine(self, who):
            return e

    s, q = Over(), (0.05, 0.5, 0.95)
    rows = e.rows * e.N
    say("# derived histories: every resident row (%d), not the window" % rows)
    for name, fn in (("ratio x[2] / x[1], n_out = 1", RATIO), ("line on 64 abscissae, n_out = 64", LINE)):
        ldd = fn.n_out + (fn.n_out & 1)
        s.derived_history(fn).close()                  # compiles if need be; first launch

        def build():
            s.derived_history(fn).close()

        t_build, _ = median_time(build)
        t_der, _ = median_time(lambda: DV.compute(e.derive, DV.single_process_allgather, fn, 0, e.N, e.rows))
        moved = rows * (e.ld + 1) * 8 + rows * (ldd + 1) * 8
        with s.derived_history(fn) as dh:
            dh.param_est_quantiles(e.n_burn, q=q)
            t_q, got = median_time(lambda: dh.param_est_quantiles(e.n_burn, q=q))
        say("%s: derived_history build (create + fill + close) host-to-host %.3f ms; it reads %.2f GB and writes %.3f GB (ln-likes included): "
            "%.2f TB/s = %.3f of 8 TB/s; bpm_derive over the same rows in this run %.3f ms (%.2f x); dh.param_est_quantiles(5 / 50 / 95 %%) %.3f ms"
            % (name, t_build * 1e3, rows * (e.ld + 1) * 8 / 1e9, rows * (ldd + 1) * 8 / 1e9, moved / t_build / 1e12, moved / t_build / PEAK_BW,
               t_der * 1e3, t_build / t_der, t_q * 1e3))
        if not device_only:
            t0 = time.perf_counter()
            V = s.param_est_fn(fn, e.n_burn, values=True).values
            want = np.quantile(V, q, axis=0)
            t_np = time.perf_counter() - t0
            say("    the parent commit's route, param_est_fn(values=True) + np.quantile: %.2f s = %.0f x build + quantiles; equal to the device: %s"
                % (t_np, t_np / (t_build + t_q), bool(np.array_equal(got, want, equal_nan=True))))
            del V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("G", nargs="?", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    report = Report()
    say = report.say
    e = cfg2_engine(a.G)
    N, d, rows, n_burn = e.N, e.d, e.rows, e.n_burn
    say("# derived quantities at cfg2's shape: N = %d chains, d = %d, %d history rows; window = rows >= %d: %d rows, %.2f GB of states; build %s"
        % (N, d, rows, n_burn, e.n, e.win_bytes / 1e9, L.build_id(e.lib)))

    def run(fn):
        return DV.compute(e.derive, DV.single_process_allgather, fn, n_burn, N, rows)

    e.reduce_moments(n_burn)
    t_mom, _ = median_time(lambda: e.reduce_moments(n_burn))
    say("(b) plain pass over the window of this build, host-to-host: bpm_reduce_moments %.3f ms (%.2f TB/s = %.3f of 8 TB/s)"
        % (t_mom * 1e3, e.win_bytes / t_mom / 1e12, e.win_bytes / t_mom / PEAK_BW))
    H = LL = None
    t_copy = 0.0
    if not a.device_only:
        t0 = time.perf_counter()
        H, LL = e.get_history(), e.get_loglike_history()
        t_copy = time.perf_counter() - t0
        say("(a) get_history() + get_loglike_history(): %.2f s (%.2f GB to the host)" % (t_copy, (H.nbytes + LL.nbytes) / 1e9))
    for name, fn in (("ratio x[2] / x[1], n_out = 1", RATIO), ("line on 64 abscissae, n_out = 64", LINE)):
        t0 = time.perf_counter()
        run(fn)                                        # compiles (hiprtc), loads the module, first launch
        t_first = time.perf_counter() - t0
        t_call, pd = median_time(lambda: run(fn))
        for kb in (40, 30, 20):                        # A/B: a smaller LDS budget per workgroup, more workgroups per CU
            os.environ["BPM_DERIVE_LDS_KB"] = str(kb)
            run(fn)
            say("    BPM_DERIVE_LDS_KB=%d: %.3f ms" % (kb, median_time(lambda: run(fn))[0] * 1e3))
        del os.environ["BPM_DERIVE_LDS_KB"]
        say("%s: param_est_fn host-to-host %.3f ms (first call with the compilation: %.2f s); the pass reads %.2f GB of states + %.3f GB of "
            "ln-likes: %.2f TB/s = %.3f of 8 TB/s; %.2f x the plain pass (b)"
            % (name, t_call * 1e3, t_first, e.win_bytes / 1e9, e.n * 8 / 1e9, e.win_bytes / t_call / 1e12, e.win_bytes / t_call / PEAK_BW,
               t_call / t_mom))
        if not a.device_only:
            t0 = time.perf_counter()
            V = fn(H.reshape(-1, d)[n_burn:], LL.reshape(-1)[n_burn:])
            mean, sd, mn, mx = V.mean(axis=0), V.std(axis=0), V.min(axis=0), V.max(axis=0)
            t_np = time.perf_counter() - t0
            say("    (a) the NumPy statement with np.mean / std / min / max over its %d x %d values: %.2f s; with the copy %.2f s = %.0f x param_est_fn"
                % (V.shape[0], V.shape[1], t_np, t_copy + t_np, (t_copy + t_np) / t_call))
            say("    min / max equal to NumPy: %s; largest |mean - np.mean| / sd: %.2e; largest |sd / np.std - 1|: %.2e"
                % (bool(np.array_equal(pd.min, mn) and np.array_equal(pd.max, mx)), float(np.max(np.abs(pd.mean - mean) / sd)),
                   float(np.max(np.abs(pd.sd / sd - 1.0)))))
            del V
    derived_history_section(e, say, a.device_only)
    e.close()
    report.write(a.out)


if __name__ == "__main__":
    main()
