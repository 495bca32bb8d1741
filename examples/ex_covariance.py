#!/usr/bin/env python3
"""How the parameters move together: the posterior covariance and correlation matrix, reduced on the GPU from the resident history
(param_est_cov), nothing of the history crossing PCIe.
  1. The shipped equicorrelated Gaussian (10 coordinates, rho = 0.5): every off-diagonal correlation comes out near rho.
  2. The banana with an uncorrelated underlying Gaussian (rho = 0): its second coordinate follows the square of the first, yet the LINEAR
     correlation a covariance matrix reports is near zero (analytically cov = [[a^2, 0], [0, 1 / a^2 + 2 b^2]]) -- a correlation matrix
     sees straight-line dependence only.  (The shipped default, rho = 0.9, has cov_01 = rho exactly: correlation 0.698.)"""
from __future__ import division, print_function

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd.demc import DeMcMpi
from bipymc_amd.dream import DreamMpi
from bipymc_amd.utils import banana_rv, d100_gauss

if __name__ == "__main__":
    n_chains, dim, gens = 256, 10, 4000
    gauss = d100_gauss.Gauss_100D(rho=0.5, dim=dim)
    sampler = DreamMpi(gauss.ln_like, np.zeros(dim), n_chains=n_chains, n_cr_gen=50, burnin_gen=200, seed=42)
    sampler.run_mcmc(n_chains * (gens + 1))
    pc = sampler.param_est_cov(n_burn=n_chains * (gens // 2))        # the second half of the history
    corr = pc.corr()
    off = corr[~np.eye(dim, dtype=bool)]
    print("equicorrelated Gaussian, rho = %.2f: %d rows; off-diagonal correlations mean %.4f, min %.4f, max %.4f"
          % (gauss.rho, pc.n, off.mean(), off.min(), off.max()))
    print("standard deviations (target sqrt(k + 1)): %s" % np.array2string(np.sqrt(np.diag(pc.cov)), precision=3))

    n_chains, gens = 512, 4000
    banana = banana_rv.Banana_2D(rho=0.0)
    sampler = DeMcMpi(banana.ln_like, np.zeros(2), n_chains=n_chains, seed=7, p_snooker=0.1)
    sampler.run_mcmc(n_chains * (gens + 1))
    pc = sampler.param_est_cov(n_burn=n_chains * (gens // 2))
    want = np.array([[banana.a ** 2, 0.0], [0.0, 1.0 / banana.a ** 2 + 2.0 * banana.b ** 2]])
    print("banana (rho = 0): covariance\n%s\nanalytic\n%s\nlinear correlation of the two coordinates %.4f: near zero, although x[1] follows "
          "x[0]^2 -- the dependence is not a straight line" % (np.array2string(pc.cov, precision=4), np.array2string(want, precision=4),
                                                                pc.corr()[0, 1]))
