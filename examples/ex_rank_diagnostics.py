#!/usr/bin/env python3
"""DE-MC with snooker updates on the shipped banana (a heavy-tailed, curved 2-D target): the classic split-R-hat / ESS beside the
rank-normalized split-R-hat, bulk-ESS and tail-ESS (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021; what Stan and ArviZ report), both
over the second half of the history and both reduced on the GPU.  The classic pair compares means and variances of the raw values; the
rank-normalized one also sees chains that differ in scale (r_hat_tail) and says how well the 5 % and 95 % quantiles -- the ends of the band
one reports -- are estimated (ess_tail).  Then the ranks themselves as a resident history, and a rank plot of two chains from it."""
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
    classic = sampler.convergence_diagnostics(n_burn=n_burn)
    t1 = time.time()
    rank = sampler.convergence_diagnostics_rank(n_burn=n_burn)
    t2 = time.time()
    print("generations %d-%d, %d half-chains of %d draws; classic %.1f ms, rank-normalized %.1f ms"
          % (rank.window[0], rank.window[1] - 1, rank.n_half_chains, rank.n_draws, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    for k in range(2):
        print("x[%d]: classic R-hat %.4f ESS %.0f | rank-normalized R-hat %.4f (bulk %.4f, tail %.4f)  ESS bulk %.0f  tail %.0f "
              "(5%%: %.0f, 95%%: %.0f)" % (k, classic.r_hat[k], classic.ess[k], rank.r_hat[k], rank.r_hat_bulk[k], rank.r_hat_tail[k],
                                         rank.ess_bulk[k], rank.ess_tail[k], rank.ess_lower[k], rank.ess_upper[k]))
        print("      median %+.4f, 5 %% %+.4f, 95 %% %+.4f" % (rank.median[k], rank.quantiles[0, k], rank.quantiles[1, k]))
    # a rank plot: the histogram of one chain's pooled ranks is flat when that chain explores what the population explores
    with sampler.rank_history(n_burn=n_burn, scale="rank") as rh:
        S = rh.history_rows * rh.n_chains
        r = rh.param_est(0)[2].reshape(rh.history_rows, rh.n_chains, 2)
        for i in (0, 1):
            counts = np.histogram(r[:, i, 0], bins=10, range=(0.5, S + 0.5))[0]
            print("chain %d, x[0]: ranks per decile (expected %d each): %s" % (i, rh.history_rows // 10, " ".join("%d" % c for c in counts)))
