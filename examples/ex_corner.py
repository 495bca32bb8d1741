#!/usr/bin/env python3
"""The numbers of a corner plot without moving the samples: the marginal histogram of every parameter and the joint histogram of a pair,
counted on the GPU from the resident history (param_est_hist) -- what corner.corner(samples) bins on the host.  The banana target: its
second coordinate follows the square of the first, which the 2-D counts show and a covariance matrix cannot.  Draws the plot only where
matplotlib is installed."""
from __future__ import division, print_function

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a checkout

from bipymc_amd.demc import DeMcMpi
from bipymc_amd.utils import banana_rv

if __name__ == "__main__":
    n_chains, gens = 512, 4000
    banana = banana_rv.Banana_2D()
    sampler = DeMcMpi(banana.ln_like, np.zeros(2), n_chains=n_chains, seed=7, p_snooker=0.1)
    sampler.run_mcmc(n_chains * (gens + 1))
    ph = sampler.param_est_hist(n_burn=n_chains * (gens // 2), bins=20, pairs="all")      # the second half of the history
    print("banana: %d rows; 20 bins per coordinate" % ph.n)
    for j, k in enumerate(ph.dims):
        print("x[%d] in [%.3f, %.3f]: counts %s" % (k, ph.edges[j, 0], ph.edges[j, -1], ph.counts[j].tolist()))
    a, b = ph.pairs[0]
    print("counts of the pair (x[%d], x[%d]), rows = bins of x[%d]:" % (a, b, a))
    print(np.array2string(ph.counts2d[0], max_line_width=200))
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("(matplotlib is not installed: no picture)")
    else:
        fig, ax = plt.subplots(2, 2, figsize=(7, 7))
        dens = ph.density()
        for j in range(2):
            ax[j, j].stairs(dens[j], ph.edges[j])
            ax[j, j].set_xlabel("x[%d]" % ph.dims[j])
        ax[1, 0].pcolormesh(ph.edges2d[0], ph.edges2d[1], ph.counts2d[0].T)
        ax[1, 0].set_xlabel("x[%d]" % a)
        ax[1, 0].set_ylabel("x[%d]" % b)
        ax[0, 1].axis("off")
        out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ex_corner.png")
        fig.savefig(out, dpi=120)
        print("wrote %s" % out)
