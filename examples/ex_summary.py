#!/usr/bin/env python3
"""DE-MC with snooker updates on the shipped banana (a heavy-tailed, curved 2-D target), then the table a Bayesian report prints -- mean, sd,
the 94 % highest-density interval, the Monte Carlo standard errors of mean and sd, bulk / tail ESS and the rank-normalized R-hat -- over the
second half of the history, every column reduced on the GPU from the resident history.  The highest-density interval is the SHORTEST interval
holding 94 % of the draws: on the banana's skewed second coordinate it is visibly not the pair of 3 % and 97 % quantiles.  The standard
errors say how many digits of mean and sd are worth printing."""
from __future__ import division, print_function

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd.demc import DeMcMpi
from bipymc_amd.utils import banana_rv

if __name__ == "__main__":
    n_chains, gens = 512, 2000
    sampler = DeMcMpi(banana_rv.Banana_2D().ln_like, np.zeros(2), n_chains=n_chains, seed=42, p_snooker=0.1)
    sampler.run_mcmc(n_chains * (gens + 1))
    n_burn = n_chains * (gens // 2)
    t0 = time.time()
    ps = sampler.posterior_summary(n_burn=n_burn, hdi_prob=0.94, prob=(0.03, 0.97))
    t1 = time.time()
    print(ps)
    print("(%.1f ms)" % ((t1 - t0) * 1e3))
    for k in range(2):
        digits = max(0, int(np.ceil(-np.log10(2.0 * ps.mcse_mean[k]))))
        print("x[%d] = %.*f +- %.*f (sd; its own standard error %.2g); 94 %% HDI [%+.3f, %+.3f] is %.3f wide, the 3 %% - 97 %% quantiles "
              "[%+.3f, %+.3f] %.3f" % (k, digits, ps.mean[k], digits, ps.sd[k], ps.mcse_sd[k], ps.hdi_lo[k], ps.hdi_hi[k],
                                       ps.hdi_hi[k] - ps.hdi_lo[k], ps.quantiles[0, k], ps.quantiles[1, k], ps.quantiles[1, k] - ps.quantiles[0, k]))
    # several intervals at once over param_est's own window: every super-chain row after n_burn
    h = sampler.param_est_hdi(n_burn=n_burn, prob=(0.5, 0.8, 0.94))
    for p, lo, hi in zip(h.prob, h.lo, h.hi):
        print("%2.0f %% HDI of %d draws: x[0] in [%+.3f, %+.3f], x[1] in [%+.3f, %+.3f]" % (100 * p, h.n, lo[0], hi[0], lo[1], hi[1]))
