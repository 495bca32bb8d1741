#!/usr/bin/env python3
"""A run longer than its history should be: DREAM on the shipped correlated Gaussian (10 coordinates), first 2000 generations with a row per
generation; convergence_diagnostics gives the integrated autocorrelation time tau of every coordinate, and rows closer together than about
tau / 2 carry little that their neighbours do not -- so the history is thinned to every k-th generation, k = tau_median / 2 (thin_history
returns the device memory of the dropped rows), and the run goes on storing every k-th generation only: 6000 more generations cost the memory
of 6000 / k.  The quantiles at the end are those of the WHOLE run's stored rows.  n_burn, lags and ESS of every statistic count stored rows
from then on; history_generations() says which generation each stored row is."""
from __future__ import division, print_function

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd.dream import DreamMpi
from bipymc_amd.utils import d100_gauss

if __name__ == "__main__":
    n_chains, dim, first, more = 256, 10, 2000, 6000
    gauss = d100_gauss.Gauss_100D(dim=dim)
    sampler = DreamMpi(gauss.ln_like, np.zeros(dim), n_chains=n_chains, n_cr_gen=50, burnin_gen=200, seed=42)
    sampler.run_mcmc(n_chains * (first + 1))
    diag = sampler.convergence_diagnostics(n_burn=n_chains * (first // 2))          # the second half: past burn-in
    tau = float(np.nanmedian(diag.tau))                                              # (a constant coordinate has no autocorrelation time: NaN)
    k = max(1, int(tau / 2)) if np.isfinite(tau) else 1
    print("%d generations, a row each: max R-hat %.4f, ESS median %.0f of %d draws, autocorrelation time median %.1f generations -> thin = %d"
          % (first, np.max(diag.r_hat), np.median(diag.ess), diag.n_half_chains * diag.n_draws, tau, k))
    rows_before = len(sampler.history_generations())
    sampler.thin_history(k)
    gens = sampler.history_generations()
    print("thin_history(%d): %d rows -> %d rows (generations %s ... %d), sampler.thin = %d"
          % (k, rows_before, len(gens), ", ".join(str(g) for g in gens[:3]), gens[-1], sampler.thin))
    sampler.run_mcmc(n_chains * (more + 1))                                          # ... and on: every k-th generation is stored
    gens = sampler.history_generations()
    print("%d generations run, %d rows stored (a row per generation would be %d)" % (first + more, len(gens), first + more + 1))
    # from here on n_burn counts STORED rows: leave out the rows of the first `first // 2` generations
    n_burn = n_chains * int(np.searchsorted(gens, first // 2))
    diag = sampler.convergence_diagnostics(n_burn=n_burn)
    print("stored rows from generation %d on: max R-hat %.4f, ESS median %.0f of %d stored draws, autocorrelation time median %.2f stored rows"
          % (gens[n_burn // n_chains], np.max(diag.r_hat), np.median(diag.ess), diag.n_half_chains * diag.n_draws, np.median(diag.tau)))
    qs = sampler.param_est_quantiles(n_burn=n_burn, q=(0.05, 0.5, 0.95))
    for j in range(dim):
        print("x[%d]: 5%% %+.4f  50%% %+.4f  95%% %+.4f   R-hat %.4f" % (j, qs[0, j], qs[1, j], qs[2, j], diag.r_hat[j]))
