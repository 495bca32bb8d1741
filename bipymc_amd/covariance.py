"""Posterior covariance and correlation of a sampler's resident history: what `np.cov(param_est(n_burn)[2], rowvar=False)` returns,
computed without moving the history off the GPU(s).

The device sums (bpm_reduce_moments, then bpm_reduce_cov: an FP64 matrix-core SYRK, bipymc_amd/csrc/covariance.h); this module chooses the
centre and merges the ranks.  Two passes over the window:
  1. every rank's shifted sums (count, S1 = sum (x - shift), shift) travel through `allgather`; every rank adds them in rank order, so the
     global mean  c = shift + S1 / n  has the same bits everywhere (and equals a constant column's constant exactly: its S1 is 0);
  2. every rank's centred sums about c, S1 = sum (x - c) and S2 = sum (x - c)(x - c)^T, travel the same way and are added in rank order;
     cov = (S2 - S1 S1^T / n) / (n - 1),  mean = c + S1 / n.
Centring on the global mean keeps |x - c| at the posterior's own scale whatever its offset, so the rounding error of S2_ij is bounded by
n u sqrt(S2_ii S2_jj) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1) instead of growing with mean^2 / variance.
"""
from __future__ import division

import collections

import numpy as np

from ._history_stats import check_n_burn, empty_window
from .comm import single_process_allgather  # noqa: F401  (for callers without a communicator)


class PosteriorCovariance(collections.namedtuple("PosteriorCovariance", ["mean", "cov", "n"])):
    """mean (dim,), cov (dim, dim) with ddof = 1, exactly symmetric; n rows of the window, summed over ranks"""
    __slots__ = ()

    def corr(self):
        """cov / sqrt(outer(diag, diag)): unit diagonal; a NaN row and column where a variance is 0 or NaN"""
        var = np.diag(self.cov)
        good = var > 0
        sd = np.sqrt(np.where(good, var, 1.0))
        c = self.cov / np.outer(sd, sd)
        c[~good, :] = np.nan
        c[:, ~good] = np.nan
        idx = np.flatnonzero(good)
        c[idx, idx] = 1.0
        return c


def finish(n, center, s1, s2):
    """the merged centred sums -> PosteriorCovariance"""
    n = int(n)
    s1 = np.asarray(s1, dtype=np.float64)
    s2 = np.asarray(s2, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cov = (s2 - np.outer(s1, s1) / n) / (n - 1)
        mean = center + s1 / n
    return PosteriorCovariance(mean, cov, n)


def compute(reduce_moments, reduce_cov, allgather, n_burn, dim):
    """The collective driver.  reduce_moments(n_burn) -> (count, S1, S2, shift) of this rank's rows (HipEngine.reduce_moments);
    reduce_cov(n_burn, center) -> (count, S1 (dim,), S2 (dim, dim)) about `center` (HipEngine.reduce_cov); allgather(obj) -> [obj of every
    rank] in rank order ([obj] for one process, single_process_allgather).  -> PosteriorCovariance, the same bits on every rank"""
    n_burn = check_n_burn("param_est_cov", n_burn)
    dim = int(dim)
    parts = [(int(p[0]), np.asarray(p[1], dtype=np.float64)) + tuple(p[2:]) for p in allgather(reduce_moments(n_burn))]
    shift = np.asarray(parts[0][3], dtype=np.float64).reshape(dim)      # (identical on every rank)
    n = sum(int(p[0]) for p in parts)
    if n < 2:
        reduce_cov(n_burn, shift)       # (a sampler without a resident history says so here rather than reporting an empty window)
        if n == 0:
            raise empty_window("param_est_cov", n_burn)
        raise ValueError("param_est_cov: a covariance needs at least 2 rows; the window after n_burn = %d holds %d" % (n_burn, n))
    tot = np.zeros(dim)
    for p in parts:
        tot = tot + p[1].reshape(dim)
    with np.errstate(invalid="ignore", over="ignore"):
        center = shift + tot / n
    parts = allgather(reduce_cov(n_burn, center))
    if sum(int(p[0]) for p in parts) != n:
        raise RuntimeError("covariance: the two passes saw different windows (the history changed between them?)")
    s1 = np.zeros(dim)
    s2 = np.zeros((dim, dim))
    with np.errstate(invalid="ignore", over="ignore"):
        for p in parts:
            s1 = s1 + np.asarray(p[1], dtype=np.float64).reshape(dim)
            s2 = s2 + np.asarray(p[2], dtype=np.float64).reshape(dim, dim)
    return finish(n, center, s1, s2)
