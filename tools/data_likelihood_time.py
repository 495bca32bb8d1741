#!/usr/bin/env python3
"""The time of a generation for a straight-line fit y = a + b t written in the PER-DATUM form of HipLikelihood (a wavefront per chunk of the data,
csrc/user_eval_data.h) against the same likelihood in the PLAIN form with its data inside params, fused into the update kernel (one lane per
chain walks all the data) -- DREAM past its burn-in, d = 2, at N chains x n_data data points = 16 x 10^5, 64 x 10^4 and 8192 x 10^3.

Every figure comes from a FRESH process (a child of this script: engine, run-time compile, warm-up, then three windows of generations each ending in a
device synchronise, the window sized to half a second; the child's figure is the median of its three windows).  Each (shape, form) gets --runs children,
the forms alternating; the record gives the median of the children and their smallest and largest figure.
"floor" is the per-datum form over ONE datum: the same three kernels and launches with nothing to sum.  The likelihood's share of a per-datum generation is
taken as generation - floor (an estimate by difference, low by whatever an all but empty likelihood kernel costs), and the effective data rate is
N x n_data x w x 8 bytes (every proposal of a generation reads all the data once) over that share.
The likelihood kernels' own times come from a kernel trace, a run of its own per shape with the profiler's slowdown kept out of the figures above:
`rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/data_likelihood_time.py --child N N_DATA data --max-gens 300`, then
`tools/rocpd_summary.py stats DIR/.../kt_results.db` (kernels bpm_user_eval_data and bpm_user_fold_data).
usage: data_likelihood_time.py [--runs 5] [--out profiles/data_likelihood.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16, 100000), (64, 10000), (8192, 1000)]
FORMS = ["data", "plain", "floor"]
W = 2
TRUTH = (0.5, 2.0)

DATA_SRC = """
__device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc) {
    const double r = y[1] - (x[0] + x[1] * y[0]);
    acc[0] += r * r * p[0];
}
__device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p) { return -0.5 * acc[0]; }
"""
PLAIN_SRC = """
__device__ double ln_like(const double* x, int d, const double* p) {      // p = [1 / sigma^2, n, t_0, y_0, t_1, y_1, ...]
    const int n = (int)p[1];
    double s = 0.0;
    for (int i = 0; i < n; ++i) { const double r = p[3 + 2 * i] - (x[0] + x[1] * p[2 + 2 * i]); s += r * r * p[0]; }
    return -0.5 * s;
}
"""


def child(N, n_data, form, max_gens=10000):
    from bipymc_amd import HipLikelihood, _lib as L
    from bipymc_amd.engine import HipEngine
    rs = np.random.RandomState(1)
    t = rs.uniform(size=n_data)
    data = np.column_stack([t, TRUTH[0] + TRUTH[1] * t + 0.3 * rs.normal(size=n_data)])
    inv_s2 = 1.0 / 0.09
    eng = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=2, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=7, burnin_gen=0)
    sd = 0.3 / np.sqrt(n_data)
    eng.set_state(np.array(TRUTH) + 3.0 * sd * rs.normal(size=(N, 2)))
    if form == "plain":
        ll = HipLikelihood(PLAIN_SRC, params=np.concatenate([[inv_s2, n_data], data.reshape(-1)]))
        eng.set_device_likelihood(ll.source, ll.params)
    else:
        ll = HipLikelihood(DATA_SRC, params=[inv_s2], data=data[:1] if form == "floor" else data, terms=1)
        eng.set_device_likelihood(ll.source, ll.params, data=ll.data)
    fused = eng.device_likelihood_info()[0]
    assert fused == (form == "plain"), eng.device_likelihood_info()

    def window(g):
        t0 = time.perf_counter()
        eng.step(g)
        eng.synchronize()
        return (time.perf_counter() - t0) / g

    eng.begin_run()
    window(5)                                                    # warm-up: every kernel of the steady state has run
    g = int(min(max_gens, max(20, 0.5 / window(10))))
    eng.reserve_history(16 + 3 * g + 8)                          # (no growth of the history inside a window)
    us = sorted(window(g) * 1e6 for _ in range(3))
    st = eng.stats()
    print(json.dumps(dict(N=N, n_data=n_data, form=form, fused=bool(fused), gens=g, us_per_gen=us[1], windows=us,
                          accept=st["local_n_accepted"] / float(st["local_n_accepted"] + st["local_n_rejected"]), build=L.build_id(eng.lib))))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_likelihood.txt"))
    ap.add_argument("--child", nargs=3, default=None, metavar=("N", "N_DATA", "FORM"))
    ap.add_argument("--max-gens", type=int, default=10000, help="generations per window at the most (a child under a kernel trace: a few hundred)")
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), int(a.child[1]), a.child[2], a.max_gens)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    build = None
    for N, n_data in SHAPES:
        res = {f: [] for f in FORMS}
        for _ in range(a.runs):
            for f in FORMS:                                      # (alternating: whatever else the machine does falls on every form alike)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N), str(n_data), f], stdout=subprocess.PIPE, timeout=300, check=True)
                r = json.loads(out.stdout.decode().strip().splitlines()[-1])
                res[f].append(r)
                build = r["build"]
        if not lines:
            say("# a generation of DREAM (d = 2, steady state) on a straight-line fit: the per-datum form (three kernels, a wavefront per 4096 data points) against "
                "the plain form with the data in params (fused into the update kernel, a lane per chain); %d fresh processes per figure, median "
                "[smallest .. largest] of their medians; build %s" % (a.runs, build))
        med = {f: float(np.median([r["us_per_gen"] for r in res[f]])) for f in FORMS}
        span = {f: (min(r["us_per_gen"] for r in res[f]), max(r["us_per_gen"] for r in res[f])) for f in FORMS}
        say("N = %d chains, n_data = %d:" % (N, n_data))
        for f in FORMS:
            say("  %-5s  %10.1f us / generation  [%.1f .. %.1f]   (%d generations per window, acceptance %.2f)"
                % (f, med[f], span[f][0], span[f][1], res[f][0]["gens"], res[f][0]["accept"]))
        like = max(med["data"] - med["floor"], 1e-3)
        byts = float(N) * n_data * W * 8
        say("  plain / per-datum = %.1f x; the plain form's own spread is %.1f %% of its median" % (med["plain"] / med["data"], 100.0 * (span["plain"][1] - span["plain"][0]) / med["plain"]))
        say("  likelihood share of a per-datum generation (generation - floor): %.1f us for %.1f MB of data read = %.1f GB/s effective"
            % (like, byts / 1e6, byts / like / 1e3))
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
