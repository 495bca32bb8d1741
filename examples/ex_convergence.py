#!/usr/bin/env python3
"""Run DREAM on the shipped correlated Gaussian (10 coordinates) in chunks of run_mcmc until split-R-hat of every coordinate is below 1.01
over the second half of the history, then report the effective sample size and the exact 5/50/95 % posterior quantiles.  Both are reduced
on the GPU: nothing of the history crosses PCIe.  (At d = 100 each chain's autocorrelation time is several hundred generations: R-hat < 1.01 takes tens of thousands.)"""
from __future__ import division, print_function

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd.dream import DreamMpi
from bipymc_amd.utils import d100_gauss

if __name__ == "__main__":
    n_chains, dim, chunk, max_chunks = 256, 10, 500, 40
    gauss = d100_gauss.Gauss_100D(dim=dim)
    sampler = DreamMpi(gauss.ln_like, np.zeros(dim), n_chains=n_chains, n_cr_gen=50, burnin_gen=200, seed=42)
    gens = 0
    for _ in range(max_chunks):
        sampler.run_mcmc(n_chains * (chunk + 1))
        gens += chunk
        t0 = time.time()
        diag = sampler.convergence_diagnostics(n_burn=n_chains * (gens // 2))     # the second half of the history
        dt = time.time() - t0
        print("%5d generations: max R-hat %.4f over generations %d-%d (%.1f ms)" % (gens, np.max(diag.r_hat), diag.window[0], diag.window[1] - 1,
                                                                                   dt * 1e3))
        if np.max(diag.r_hat) < 1.01:
            break
    else:
        print("max R-hat still %.4f after %d generations" % (np.max(diag.r_hat), gens))
    print("ESS per coordinate: min %.0f, median %.0f, max %.0f of %d draws (%d half-chains x %d); integrated autocorrelation time "
          "median %.1f" % (np.min(diag.ess), np.median(diag.ess), np.max(diag.ess), diag.n_half_chains * diag.n_draws, diag.n_half_chains,
                           diag.n_draws, np.median(diag.tau)))
    # 5 / 50 / 95 % posterior quantiles of the same window, exact (np.quantile over param_est's rows), next to R-hat
    qs = sampler.param_est_quantiles(n_burn=n_chains * (gens // 2), q=(0.05, 0.5, 0.95))
    for k in range(dim):
        print("x[%d]: 5%% %+.4f  50%% %+.4f  95%% %+.4f   R-hat %.4f" % (k, qs[0, k], qs[1, k], qs[2, k], diag.r_hat[k]))
