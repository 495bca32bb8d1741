#!/usr/bin/env python3
"""A trace plot without moving the history: per generation the population's mean, its one-sd band and its envelope, the climb of the
log-likelihood, a handful of individual chains and the best sample seen, reduced on the GPU from the resident history (param_est_trace)
-- what the reference draws from param_est(n_burn=0)'s copy of every chain (plot_mcmc_indep_chains, mc_plot/mc_plot.py:52-102).  This is
also where n_burn for the other statistics is read off: the generation after which the band stops moving.  Draws the plot only where
matplotlib is installed."""
from __future__ import division, print_function

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd.demc import DeMcMpi
from bipymc_amd.utils import banana_rv

if __name__ == "__main__":
    n_chains, gens = 512, 2000
    banana = banana_rv.Banana_2D()
    sampler = DeMcMpi(banana.ln_like, np.full(2, 4.0), n_chains=n_chains, seed=7, p_snooker=0.1)      # started away from the mode
    sampler.run_mcmc(n_chains * (gens + 1))
    pt = sampler.param_est_trace(n_burn=0, every=20, chains=[0, 1, 2, n_chains - 1])
    lo, hi = pt.band()
    print("banana: %d bins of 20 generations x %d chains" % (len(pt.gen), n_chains))
    print("  gen    mean x[0]   sd x[0]    min x[0]    max x[0]   mean x[1]   sd x[1]    mean ln L     max ln L")
    for t in range(0, len(pt.gen), max(1, len(pt.gen) // 20)):
        print("%5d  %10.4f %9.4f  %10.4f  %10.4f  %10.4f %9.4f  %11.4f  %11.4f"
              % (pt.gen[t], pt.mean[t, 0], pt.sd[t, 0], pt.min[t, 0], pt.max[t, 0], pt.mean[t, 1], pt.sd[t, 1], pt.ll_mean[t], pt.ll_max[t]))
    print("best sample: ln L = %.6f at super-chain row %d (generation %d, chain %d): x = %s"
          % (pt.best_ll, pt.best_row, pt.best_row // n_chains, pt.best_row % n_chains, pt.best_x.tolist()))
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("(matplotlib is not installed: no picture)")
    else:
        fig, ax = plt.subplots(3, 1, figsize=(8, 9), sharex=True)
        for k in range(2):
            ax[k].fill_between(pt.gen, pt.min[:, k], pt.max[:, k], color="0.9", label="min ... max")
            ax[k].fill_between(pt.gen, lo[:, k], hi[:, k], color="0.7", label="mean +/- sd")
            ax[k].plot(pt.gen, pt.mean[:, k], color="k", label="mean")
            for j, c in enumerate(pt.chains):
                ax[k].plot(pt.gen, pt.chain_x[:, j, k], lw=0.7, label="chain %d" % c)
            ax[k].set_ylabel("x[%d]" % k)
        ax[0].legend(ncol=4, fontsize=7)
        ax[2].fill_between(pt.gen, pt.ll_min, pt.ll_max, color="0.9")
        ax[2].plot(pt.gen, pt.ll_mean, color="k")
        ax[2].set_ylabel("ln L")
        ax[2].set_xlabel("generation")
        out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ex_trace.png")
        fig.savefig(out, dpi=120)
        print("wrote %s" % out)
