#!/usr/bin/env python3
"""A model with a few parameters fitted to many data points: the per-datum form of HipLikelihood.

What the reference's fitting scripts do inside their Python ln_like_fn -- `-0.5 * np.sum((y - model)**2 * inv_sigma2)` over the data
(examples/ex_para_fit.py:39-72) -- written as two short HIP functions: one adds a single datum's term, the other turns the sums into the
ln-likelihood (and holds the prior).  The data go to the device once; every proposal is then summed by as many wavefronts as the data have chunks,
so 16 chains keep the device busy where the plain form (examples/ex_hip_likelihood.py) walks all the data on one lane per chain.
A parabola y = a + b t + c t^2 with known noise, 5000 data points, 16 chains."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd import DreamMpi, HipLikelihood          # noqa: E402

rs = np.random.RandomState(0)
SIGMA = 0.5
ts = np.sort(rs.uniform(-2.0, 2.0, size=5000))
ys = 1.0 - 0.7 * ts + 0.3 * ts * ts + SIGMA * rs.standard_normal(ts.size)

SRC = """
__device__ void ln_like_datum(const double* th, int d, const double* y, int i, const double* p, double* acc) {      // y = (t_i, y_i)
    const double r = y[1] - (th[0] + th[1] * y[0] + th[2] * (y[0] * y[0]));
    acc[0] += r * r;
}
__device__ double ln_like_total(const double* th, int d, const double* acc, int n_data, const double* p) {
    if (th[2] < -10.0 || th[2] > 10.0) return -INFINITY;                  // a flat prior on the curvature
    return -0.5 * acc[0] * p[0];                                          // p = [1 / sigma^2]
}
"""


def ln_like(theta):      # the same function for the host (HipLikelihood's python_fn)
    if theta[2] < -10.0 or theta[2] > 10.0:
        return -np.inf
    r = ys - (theta[0] + theta[1] * ts + theta[2] * (ts * ts))
    return -0.5 * np.sum(r * r) / SIGMA ** 2


def main():
    ll = HipLikelihood(SRC, params=[1.0 / SIGMA ** 2], data=np.column_stack([ts, ys]), terms=1, python_fn=ln_like)
    sampler = DreamMpi(ll, theta_0=np.array([0.0, 0.0, 0.0]), varepsilon=1e-2, n_chains=16, n_cr_gen=50, burnin_gen=500, seed=1)
    sampler.run_mcmc(16 * 4000)
    mean, std, chain = sampler.param_est(n_burn=16 * 2000)
    print("a = %.3f +- %.3f   b = %.3f +- %.3f   c = %.3f +- %.3f" % (mean[0], std[0], mean[1], std[1], mean[2], std[2]))
    print(sampler.posterior_summary(n_burn=16 * 2000))
    return mean, std


if __name__ == "__main__":
    main()
