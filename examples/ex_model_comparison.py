#!/usr/bin/env python3
"""Which of two models predicts the data better: a straight line against a parabola on the same data, compared by WAIC.

Both models are fitted with the per-datum form of HipLikelihood (examples/ex_data_likelihood.py); the question the fitting scripts of the
reference leave open after `param_est` -- is the curvature term worth its parameter? -- is answered from the pointwise log predictive
density: per datum the log of the posterior mean of its density and the posterior variance of its log density, reduced on the device over
the resident history (sampler.param_est_waic), then compared on the host (compare_waic).  The data are drawn from a parabola with a small
curvature: the parabola's elpd is higher by several standard errors."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd import DreamMpi, HipLikelihood, HipPointwise, compare_waic          # noqa: E402

rs = np.random.RandomState(0)
SIGMA = 0.5
ts = np.sort(rs.uniform(-2.0, 2.0, size=2000))
ys = 1.0 - 0.7 * ts + 0.15 * ts * ts + SIGMA * rs.standard_normal(ts.size)
DATA = np.column_stack([ts, ys])
INV_S2 = 1.0 / SIGMA ** 2

# model(th, t): the one line the two models differ in
MODELS = {"line": ("th[0] + th[1] * y[0]", 2), "parabola": ("th[0] + th[1] * y[0] + th[2] * (y[0] * y[0])", 3)}

FIT_SRC = """
__device__ void ln_like_datum(const double* th, int d, const double* y, int i, const double* p, double* acc) {      // y = (t_i, y_i)
    const double r = y[1] - (%s);
    acc[0] += r * r;
}
__device__ double ln_like_total(const double* th, int d, const double* acc, int n_data, const double* p) { return -0.5 * acc[0] * p[0]; }
"""
# the log density of ONE datum, its constants included (p = [1 / sigma^2]; 1.8378... = log(2 pi))
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
    mean, std, _ = sampler.param_est(n_burn=n_chains * gens // 2)
    w = sampler.param_est_waic(HipPointwise(POINT_SRC % model, data=DATA, params=[INV_S2]), n_burn=n_chains * gens // 2)
    print("%s: theta = %s +- %s" % (name, np.round(mean, 3), np.round(std, 3)))
    print(w)
    return w


def main():
    w_line, w_para = fit_and_score("line"), fit_and_score("parabola")
    diff, se = compare_waic(w_para, w_line)
    print("elpd(parabola) - elpd(line) = %.2f +- %.2f  (%s)" % (diff, se, "the parabola predicts better" if diff > 2 * se else
                                                                  "the line predicts better" if diff < -2 * se else "no clear difference"))
    return diff, se


if __name__ == "__main__":
    main()
