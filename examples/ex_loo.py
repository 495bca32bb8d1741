#!/usr/bin/env python3
"""A line against a parabola on the same data with ONE planted outlier: WAIC warns, PSIS-LOO's pareto_k points at the datum.

examples/ex_model_comparison.py compares the two models by WAIC.  Here one datum is moved far off the curve.  Its log density then varies
so much over the posterior (it sits at the end of the abscissae, where the fitted curve moves most) that p_waic_i > 0.4 -- the condition under which WAIC is not to be trusted -- and WAIC has nothing more to say.
sampler.param_est_loo re-weights the draws per datum instead (Pareto smoothed importance sampling), still without ever forming the draws x
data matrix, and reports per datum the fitted shape pareto_k: the planted datum is the one above 0.7, every other datum is far below, and
the comparison of the two models (compare_loo) stands on the data that can be trusted."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd import DreamMpi, HipLikelihood, HipPointwise, compare_loo, compare_waic          # noqa: E402

rs = np.random.RandomState(0)
SIGMA = 0.5
ts = np.sort(rs.uniform(-2.0, 2.0, size=60))
ys = 1.0 - 0.7 * ts + 0.15 * ts * ts + SIGMA * rs.standard_normal(ts.size)
OUTLIER = 59                      # the last abscissa: an outlier WITH leverage
ys[OUTLIER] += 12.0 * SIGMA
DATA = np.column_stack([ts, ys])
INV_S2 = 1.0 / SIGMA ** 2

MODELS = {"line": ("th[0] + th[1] * y[0]", 2), "parabola": ("th[0] + th[1] * y[0] + th[2] * (y[0] * y[0])", 3)}

FIT_SRC = """
__device__ void ln_like_datum(const double* th, int d, const double* y, int i, const double* p, double* acc) {      // y = (t_i, y_i)
    const double r = y[1] - (%s);
    acc[0] += r * r;
}
__device__ double ln_like_total(const double* th, int d, const double* acc, int n_data, const double* p) { return -0.5 * acc[0] * p[0]; }
"""
POINT_SRC = """
__device__ double ln_like_point(const double* th, int d, const double* y, int i, const double* p) {
    const double r = y[1] - (%s);
    return -0.5 * (r * r * p[0] - log(p[0]) + 1.8378770664093453);
}"""


def fit_and_score(name, n_chains=16, gens=4000):
    model, dim = MODELS[name]
    like = HipLikelihood(FIT_SRC % model, params=[INV_S2], data=DATA, terms=1)
    sampler = DreamMpi(like, theta_0=np.zeros(dim), varepsilon=1e-2, n_chains=n_chains, n_cr_gen=50, burnin_gen=500, seed=1)
    sampler.run_mcmc(n_chains * gens)
    n_burn = n_chains * gens // 2
    pw = HipPointwise(POINT_SRC % model, data=DATA, params=[INV_S2])
    w = sampler.param_est_waic(pw, n_burn=n_burn)
    loo = sampler.param_est_loo(pw, n_burn=n_burn)
    print("---- %s ----" % name)
    print("WAIC: elpd_waic %.2f, data with p_waic_i > 0.4: %d%s" % (w.elpd_waic, w.n_high_var, "  <- WAIC is unreliable here" if w.n_high_var else ""))
    print(loo)
    return w, loo


def main():
    (w_line, loo_line), (w_para, loo_para) = fit_and_score("line"), fit_and_score("parabola")
    for name, loo in (("line", loo_line), ("parabola", loo_para)):
        worst = int(np.nanargmax(loo.pareto_k))
        print("%s: the largest pareto_k is %.2f at datum %d (the planted one: %d)" % (name, loo.pareto_k[worst], worst, OUTLIER))
    diff, se = compare_loo(loo_para, loo_line)
    print("PSIS-LOO: elpd(parabola) - elpd(line) = %.2f +- %.2f" % (diff, se))
    diff_w, se_w = compare_waic(w_para, w_line)
    print("WAIC:     elpd(parabola) - elpd(line) = %.2f +- %.2f" % (diff_w, se_w))
    return loo_line, loo_para


if __name__ == "__main__":
    main()
