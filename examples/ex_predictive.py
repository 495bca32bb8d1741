#!/usr/bin/env python3
"""The posterior of a function of the parameters without moving the history: a derived quantity and a posterior-predictive band from
`param_est_fn` (bipymc_amd.HipFunction), then -- `derived_history` -- the 5 / 50 / 95 % quantile band of the same curve and the split
R-hat / effective sample size of the ratio itself.

The reference's fitting scripts end by copying the samples to the host and running a function over them (examples/ex_exp_fit.py:176-202: a
ratio of two parameters with its mean and standard deviation, the fitted model at every sample for the band).  Here the function is a few
lines of HIP, compiled once (hiprtc) around a reduction over the resident history: a straight-line fit y = m x + c with unknown noise as in
ex_hip_likelihood.py, then the x-intercept -c / m and the fitted line on 64 abscissae with its 2-sigma band."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd import DreamMpi, HipFunction, HipLikelihood          # noqa: E402

rs = np.random.RandomState(0)
xs = np.linspace(0.0, 10.0, 200)
ys = 1.7 * xs - 0.4 + 0.8 * rs.standard_normal(xs.size)
grid = np.linspace(-2.0, 12.0, 64)                                   # where the band is drawn: beyond the data on both sides

LN_LIKE = """
__device__ double ln_like(const double* th, int d, const double* p) {      // th = (m, c, log sigma); p = [n, x_0 .. x_{n-1}, y_0 .. y_{n-1}]
    const int n = (int)p[0];
    const double m = th[0], c = th[1], ls = th[2];
    if (ls < -5.0 || ls > 5.0) return -INFINITY;
    const double is2 = exp(-2.0 * ls);
    double s = 0.0;
    for (int i = 0; i < n; ++i) { const double r = p[1 + n + i] - (m * p[1 + i] + c); s += r * r; }
    return -0.5 * s * is2 - n * ls;
}
"""
DERIVE = """
__device__ void derive(const double* th, int d, double ll, const double* p, double* out) {      // p = the 64 abscissae
    out[0] = -th[1] / th[0];                                         // where the line crosses y = 0
    out[1] = exp(th[2]);                                             // sigma itself, not its logarithm
    for (int k = 0; k < 64; ++k) out[2 + k] = th[0] * p[k] + th[1];  // the fitted line
}
"""


def main():
    N = 4096
    sampler = DreamMpi(HipLikelihood(LN_LIKE, params=np.concatenate([[xs.size], xs, ys])), theta_0=np.array([1.0, 0.0, 0.0]), varepsilon=1e-2,
                       n_chains=N, n_cr_gen=50, burnin_gen=300, seed=1)
    sampler.run_mcmc(N * 1500)
    fn = HipFunction(DERIVE, n_out=66, params=grid)
    pd = sampler.param_est_fn(fn, n_burn=N * 700)
    print("%d samples; x-intercept = %.3f +- %.3f in [%.3f, %.3f]; sigma = %.3f +- %.3f"
          % (pd.n, pd.mean[0], pd.sd[0], pd.min[0], pd.max[0], pd.mean[1], pd.sd[1]))
    lo, hi = pd.band(2.0)
    for k in (0, 21, 42, 63):
        print("  y(%5.2f) = %7.3f   2-sigma band [%7.3f, %7.3f]   envelope [%7.3f, %7.3f]"
              % (grid[k], pd.mean[2 + k], lo[2 + k], hi[2 + k], pd.min[2 + k], pd.max[2 + k]))
    # the values themselves, if a picture needs them: one row per sample, in param_est's order
    tail = sampler.param_est_fn(fn, n_burn=N * 1499, values=True)
    print("values of the last %d samples: %r" % (tail.n, tail.values.shape))
    # A derived history is a history: the values stay on the GPU as the history of a second handle, and every statistic of the sampler
    # answers about them -- the band a skewed output needs is a quantile band, and convergence is checked on the quantity one reports.
    with sampler.derived_history(fn) as dh:
        q05, q50, q95 = dh.param_est_quantiles(N * 700, q=(0.05, 0.5, 0.95))
        cd = dh.convergence_diagnostics(N * 700)
        print("x-intercept: median %.3f, 5-95 %% band [%.3f, %.3f]; split R-hat %.4f, ESS %.0f of %d draws"
              % (q50[0], q05[0], q95[0], cd.r_hat[0], cd.ess[0], cd.n_half_chains * cd.n_draws))
        for k in (0, 21, 42, 63):
            print("  y(%5.2f): median %7.3f   5-95 %% band [%7.3f, %7.3f]   R-hat %.4f" % (grid[k], q50[2 + k], q05[2 + k], q95[2 + k], cd.r_hat[2 + k]))
    return pd


if __name__ == "__main__":
    main()
