#!/usr/bin/env python3
"""What param_est_waic costs, at the three straight-line-fit shapes of profiles/data_likelihood.txt, beside two yardsticks that are not the
pointwise kernel.  Writes profiles/waic_cfg2.txt (or the path given).

    python tools/waic_time.py [OUT.txt] [--gens G]

Per shape (N chains, n_data data points), a DREAM run of G generations on the per-datum HipLikelihood of the fit, then over the window of all
stored rows:
  waic      sampler-side param_est_waic of the pointwise normal density (one exp-free log density per (row, datum), then the online
            log-sum-exp: one exp each): median wall time of 3 calls after a warm-up that compiles, and evaluations (rows x n_data) per second;
  host (a)  the route there was before: get_history() to the host and scipy.special.logsumexp / np.var / np.mean over the (rows, n_data)
            matrix, on a window cut down until the matrix holds at most 2e7 values, scaled to evaluations per second;
  eval (b)  eval_device_likelihood of the per-datum HipLikelihood (the last merged change's kernels) over the same rows and data: as many
            calls of the caller's function, without the exp and without per-datum results; its time includes sending the rows from the host.
and the register / scratch figures of the kernels: bpm_pointwise_rows compiled off line for w = 2 (hipcc -Rpass-analysis=kernel-resource-usage
on the program text the library hands hiprtc), pw_fold_kernel and a digest of the update kernels' figures from tools/kernel_resources.py."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(8192, 1000), (64, 10000), (16, 100000)]
TRUTH = (1.0, 2.0)
POINT_SRC = """
__device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p) {
    const double r = y[1] - (x[0] + x[1] * y[0]);
    return -0.5 * (r * r * p[0] - log(p[0]) + 1.8378770664093453);
}"""
DATA_SRC = """
__device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc) {
    const double r = y[1] - (x[0] + x[1] * y[0]);
    acc[0] += r * r * p[0];
}
__device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p) { return -0.5 * acc[0]; }
"""


def _point_py(X, Y, p):
    r = Y[None, :, 1] - (X[:, 0:1] + X[:, 1:2] * Y[None, :, 0])
    return -0.5 * (r * r * p[0] - np.log(p[0]) + 1.8378770664093453)


def _median_time(f, reps=3):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def shape(N, n_data, gens):
    from scipy.special import logsumexp
    from bipymc_amd import HipLikelihood, HipPointwise
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _history_cases import _over
    rs = np.random.RandomState(5)
    t = rs.uniform(0.0, 1.0, size=n_data)
    data = np.column_stack([t, TRUTH[0] + TRUTH[1] * t + 0.3 * rs.normal(size=n_data)])
    inv_s2 = 1.0 / 0.09
    eng = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=2, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=7, burnin_gen=0)
    eng.set_state(np.array(TRUTH) + 3.0 * (0.3 / np.sqrt(n_data)) * rs.normal(size=(N, 2)))
    ll = HipLikelihood(DATA_SRC, params=[inv_s2], data=data, terms=1)
    eng.set_device_likelihood(ll.source, ll.params, data=ll.data)
    eng.begin_run()
    eng.step(gens)
    s = _over(eng)
    pw = HipPointwise(POINT_SRC, data=data, params=[inv_s2], python_fn=_point_py)
    rows = eng.history_rows() * N
    evals = float(rows) * n_data
    res = s.param_est_waic(pw, 0)
    t_waic = _median_time(lambda: s.param_est_waic(pw, 0))
    T, R, parts, per_part = eng.pointwise_layout(rows, n_data, 2)
    # (a) the host route on a window cut down until the matrix fits
    cut = int(max(1, min(rows, 2e7 // n_data)))

    def host():
        W = eng.get_history().reshape(-1, 2)[rows - cut:]
        M = pw(W)
        return logsumexp(M, axis=0) - np.log(len(M)), np.var(M, axis=0), np.mean(M, axis=0)

    t_host = _median_time(host, reps=1)
    # (b) the per-datum likelihood's own kernels over the same rows
    X = eng.get_history().reshape(-1, 2)
    t_eval = _median_time(lambda: eng.eval_device_likelihood(X))
    eng.close()
    out = ["N = %d chains, n_data = %d, %d stored generations: %d rows, %.3g evaluations; launch: %d data tiles x %d parts of %d rows, R = %d"
           % (N, n_data, rows // N, rows, evals, -(-n_data // T), parts, per_part, R),
           "  param_est_waic            %9.2f ms   %.3g evaluations / s   (elpd_waic %.6g, p_waic %.4g, se %.4g)"
           % (1e3 * t_waic, evals / t_waic, res.elpd_waic, res.p_waic, res.se),
           "  (a) host, %7d rows    %9.2f ms   %.3g evaluations / s   -> param_est_waic is %.1f x the host's rate"
           % (cut, 1e3 * t_host, cut * n_data / t_host, (evals / t_waic) / (cut * n_data / t_host)),
           "  (b) eval_device_likelihood %8.2f ms   %.3g evaluations / s   -> param_est_waic takes %.2f x its time"
           % (1e3 * t_eval, evals / t_eval, t_waic / t_eval)]
    return out


def rtc_resources(w=2):
    """VGPRs / scratch of bpm_pointwise_rows for POINT_SRC, compiled off line as the library hands it to hiprtc"""
    csrc = os.path.join(ROOT, "bipymc_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "pw.hip")
        with open(src, "w") as f:
            f.write("#define BPM_POINTWISE_W %d\n%s\n#include \"pointwise_rows.h\"\n" % (w, POINT_SRC))
        r = subprocess.run(["hipcc", "-x", "hip", "-include", "hip/hip_runtime.h", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--cuda-device-only", "-c",
                            "-I", csrc, "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(td, "pw.co")], capture_output=True, text=True)
    keep, name = [], None
    for line in r.stderr.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
        for key in ("VGPRs:", "ScratchSize [bytes/lane]:", "Occupancy [waves/SIMD]:"):
            if key in line and name == "bpm_pointwise_rows":
                keep.append(key + " " + line.split(key)[1].split()[0])
    return "bpm_pointwise_rows (w = %d, the straight-line density): %s" % (w, ", ".join(keep) if keep else "not compiled: " + r.stderr[-300:])


def library_resources():
    """pw_fold_kernel's figures, and a digest of the update kernels' (compare it with the same line of the parent commit's library:
    python tools/kernel_resources.py LIB phase_fused lists them one by one)"""
    import hashlib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    ks = sorted(kernel_resources(os.path.join(ROOT, "bipymc_amd", "libbipymc_hip.so")), key=lambda k: k["name"])
    out = ["pw_fold_kernel: VGPRs %d, scratch %d, LDS %d" % (k["vgpr"], k["priv"], k["lds"]) for k in ks if "pw_fold_kernel" in k["name"]]
    upd = ["%s %d %d %d %d %d" % (k["name"], k["vgpr"], k["agpr"], k["sgpr"], k["priv"], k["lds"]) for k in ks if "phase_fused_kernel" in k["name"]]
    out.append("update kernels (phase_fused_kernel): %d instantiations, sha256 of their name / VGPR / AGPR / SGPR / scratch / LDS lines %s"
               % (len(upd), hashlib.sha256("\n".join(upd).encode()).hexdigest()[:16]))
    return out


def main(argv):
    gens = int(argv[argv.index("--gens") + 1]) if "--gens" in argv else 300
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--gens")]
    out_path = paths[0] if paths else os.path.join(ROOT, "profiles", "waic_cfg2.txt")
    from bipymc_amd import _lib as L
    lines = ["# param_est_waic at the straight-line-fit shapes of profiles/data_likelihood.txt (tools/waic_time.py; wall time, median of 3 calls after a warm-up); build %s"
             % L.build_id(L.load())]
    for N, n_data in SHAPES:
        lines += shape(N, n_data, gens if N < 8192 else min(gens, 200))
        print("\n".join(lines[-4:]), flush=True)
    lines.append("# kernel resources (code-object metadata; no GPU needed)")
    lines.append(rtc_resources())
    lines += library_resources()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-12:]))


if __name__ == "__main__":
    main(sys.argv[1:])
