#!/usr/bin/env python3
"""The cost of param_est_loo beside param_est_waic on the same window, at cfg2's shape (profiles/waic_cfg2.txt's first: N = 8192 chains,
1000 data points of the straight-line fit, 201 stored generations) and at the shape with many data (64 chains, 10^4 data).

    python tools/loo_time.py [OUT]              # needs a GPU; default OUT: profiles/loo_cfg2.txt
    python tools/loo_time.py --resources [OUT]  # the kernels' registers / scratch / LDS only: no GPU needed

Per shape: the wall time of param_est_waic and of param_est_loo (median of 3 calls after a warm-up; param_est_loo calls the WAIC path once for
lppd_i, so its time holds that too), and the device time of the three stages from the call's own event pairs (stats: tail_us = selection +
merge of the row parts + sort, body_us = the second pass, fit_us = the fit and the finish), with the launch the layout chose.  Then the
registers, scratch and LDS of the run-time kernels (compiled off line, as the library hands them to hiprtc) and of the library's two."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from waic_time import DATA_SRC, POINT_SRC, TRUTH, _median_time, _point_py  # noqa: E402

SHAPES = [(8192, 1000, 200), (64, 10000, 300)]


def shape(N, n_data, gens):
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
    w = s.param_est_waic(pw, 0)
    t_waic = _median_time(lambda: s.param_est_waic(pw, 0))
    t0 = time.perf_counter()
    res = s.param_est_loo(pw, 0)                 # (the first call compiles the second run-time module)
    t_first = time.perf_counter() - t0
    runs = []

    def once():
        runs.append(s.param_est_loo(pw, 0).stats)

    t_loo = _median_time(once)
    st = runs[-1]
    med = {k: float(np.median([r[k] for r in runs[1:]])) for k in ("tail_us", "body_us", "fit_us")}
    eng.close()
    return ["N = %d chains, n_data = %d, %d stored generations: %d rows; kept sets of %d; stage A: %d data batch(es), %d row parts, at most %d compactions "
            "per workgroup; stage B: %d parts of %d rows; scratch budget %.0f MiB"
            % (N, n_data, rows // N, rows, st["k_max"], st["batches"], st["tail_parts"], st["compactions"], st["body_parts"], st["body_rows_per_part"],
               st["budget_bytes"] / 2.0 ** 20),
            "  param_est_waic            %9.2f ms   (elpd_waic %.6g, p_waic %.4g, data with p_waic_i > 0.4: %d)" % (1e3 * t_waic, w.elpd_waic, w.p_waic, w.n_high_var),
            "  param_est_loo             %9.2f ms   (elpd_loo %.6g, p_loo %.4g, data with pareto_k > 0.7: %d; the first call, with the compilation: %.0f ms)"
            % (1e3 * t_loo, res.elpd_loo, res.p_loo, res.n_bad_k, 1e3 * t_first),
            "    on the device: A (select, merge, sort) %9.2f ms | B (body log-sum-exp) %9.2f ms | C (fit and finish) %9.2f ms   -> param_est_loo takes %.1f x "
            "param_est_waic's time" % (1e-3 * med["tail_us"], 1e-3 * med["body_us"], 1e-3 * med["fit_us"], t_loo / t_waic)]


def rtc_resources(w=2):
    """registers / scratch / LDS of pointwise_tail.h's kernels around POINT_SRC, compiled off line as the library hands them to hiprtc"""
    csrc = os.path.join(ROOT, "bipymc_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "pt.hip")
        with open(src, "w") as f:
            f.write("#define BPM_POINTWISE_W %d\n%s\n#include \"pointwise_tail.h\"\n" % (w, POINT_SRC))
        r = subprocess.run(["hipcc", "-x", "hip", "-include", "hip/hip_runtime.h", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--cuda-device-only", "-c",
                            "-I", csrc, "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(td, "pt.co")], capture_output=True, text=True)
    found, name = {}, None
    for line in r.stderr.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
        for key in ("VGPRs:", "ScratchSize [bytes/lane]:", "Occupancy [waves/SIMD]:", "LDS Size [bytes/block]:"):
            if key in line and name:
                found.setdefault(name, []).append(key + " " + line.split(key)[1].split()[0])
    if not found:
        return ["pointwise_tail.h: not compiled: " + r.stderr[-300:]]
    return ["%s (w = %d, the straight-line density): %s" % (k, w, ", ".join(v)) for k, v in found.items()]


def library_resources():
    from kernel_resources import kernel_resources
    ks = sorted(kernel_resources(os.path.join(ROOT, "bipymc_amd", "libbipymc_hip.so")), key=lambda k: k["name"])
    return ["%s: VGPRs %d, scratch %d, LDS %d" % (n, k["vgpr"], k["priv"], k["lds"]) for n in ("pw_psis_kernel", "pw_tail_values_kernel") for k in ks
            if n in k["name"]]


def main(argv):
    only = "--resources" in argv
    paths = [a for a in argv if not a.startswith("--")]
    out_path = paths[0] if paths else os.path.join(ROOT, "profiles", "loo_cfg2.txt")
    from bipymc_amd import _lib as L
    lines = ["# param_est_loo beside param_est_waic on the same window (tools/loo_time.py; wall time, median of 3 calls after a warm-up; stages: the call's own "
             "event pairs on the device); build %s" % L.build_id(L.load())]
    if only:
        lines.append("# timing: not measured yet (python tools/loo_time.py on a GPU)")
    else:
        for N, n_data, gens in SHAPES:
            lines += shape(N, n_data, gens)
            print("\n".join(lines[-4:]), flush=True)
    lines.append("# kernel resources (code-object metadata; no GPU needed)")
    lines += rtc_resources()
    lines += library_resources()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1:])
