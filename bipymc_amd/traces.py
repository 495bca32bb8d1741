"""Per-generation trace summaries of a sampler's resident history: what a trace plot needs (the reference draws one line per chain from
`param_est(n_burn=0)`'s copy of the whole history and np.mean / np.std per generation, plot_mcmc_indep_chains / plot_mcmc_chain,
mc_plot/mc_plot.py:52-102), computed without moving the history off the GPU(s): per bin of `every` generations the centre, spread and
envelope of the population and of its log-likelihood, the best sample of the window, and the decimated traces of a handful of chains.

The device reduces (bpm_trace_bins / bpm_trace_chains, bipymc_amd/csrc/traces.h); this module validates, merges the ranks in rank order and
finishes mean and sd.  A rank hands over, per (bin, coordinate), the count n_r of its finite values, a shift c_r that is one of them and
the shifted sums S1_r = sum (x - c_r), S2_r = sum (x - c_r)^2; then mean_r = c_r + S1_r / n_r, M2_r = S2_r - S1_r^2 / n_r, and the ranks
combine by Chan et al.'s pairwise formula (merge_moments).  NumPy's rules for what is not finite are restated around that: a bin with a NaN has mean = sd =
NaN, one with an infinity has that infinity as its mean (NaN with both) and sd = NaN; min and max ignore NaN (np.nanmin / np.nanmax) and are
NaN where every value is.  Every rank runs the same arithmetic on the same gathered parts in the same order: every rank returns the same bits.
"""
from __future__ import division

import collections

import numpy as np

from ._history_stats import check_n_burn, empty_window
from .comm import single_process_allgather  # noqa: F401  (for callers without a communicator)
from .diagnostics import window

WHO = "param_est_trace"


class PosteriorTrace(collections.namedtuple("PosteriorTrace", [
        "gen", "n", "mean", "sd", "min", "max", "n_nan", "ll_mean", "ll_min", "ll_max", "best_ll", "best_x", "best_row", "chains", "chain_x",
        "chain_ll"])):
    """T bins of `every` generations (the last may be shorter), pooled over all chains.  gen (T,) int64: first generation of each bin; n (T,)
    int64: rows pooled; mean, sd (ddof 0), min, max (T, dim); n_nan (T, dim) int64; ll_mean, ll_min, ll_max (T,): the same over the
    log-likelihoods; best_ll, best_x (dim,), best_row: the window's largest log-likelihood that is not NaN, its row of the super chain and
    that row's index g * n_chains + i (the smallest on a tie; NaN, NaN, -1 where every log-likelihood is NaN); chains (C,), chain_x
    (T, C, dim), chain_ll (T, C): the requested chains at the first generation of every bin"""
    __slots__ = ()

    def band(self, k=1.0):
        """(mean - k sd, mean + k sd)"""
        return self.mean - k * self.sd, self.mean + k * self.sd


def check_every(every):
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)):
        raise TypeError("%s: every must be an integer (got %r)" % (WHO, every))
    if int(every) < 1:
        raise ValueError("%s: every must be >= 1 (got %d)" % (WHO, int(every)))
    return int(every)


def check_chains(chains, n_chains):
    """-> (C,) int64 global chain ids: none for None, else distinct ids in [0, n_chains) in the order given"""
    if chains is None:
        return np.zeros(0, dtype=np.int64)
    c = np.asarray(chains)
    if c.size == 0:
        return np.zeros(0, dtype=np.int64)
    if c.ndim != 1 or c.dtype.kind not in "iu":
        raise ValueError("%s: chains must be None or a sequence of chain indices" % WHO)
    c = c.astype(np.int64)
    if c.min() < 0 or c.max() >= n_chains:
        raise ValueError("%s: chains must lie in [0, %d)" % (WHO, n_chains))
    if len(np.unique(c)) != len(c):
        raise ValueError("%s: chains must be distinct" % WHO)
    return c


def owner_of(chains, n_chains, world_size):
    """(rank, local chain) of global chain ids: rank r holds the chains [r n_local, (r + 1) n_local), n_local = n_chains // world_size"""
    n_local = int(n_chains) // int(world_size)
    c = np.asarray(chains, dtype=np.int64)
    return c // n_local, c % n_local


def merge_moments(parts):
    """parts: per rank (n, c, S1, S2) arrays of one shape, in rank order -> (n int64, mean, M2) of the pooled finite values (mean = M2 = 0
    where there is none).  Per rank off_r = S1_r / n_r (mean_r = c_r + off_r) and M2_r = S2_r - S1_r^2 / n_r, then Chan et al.'s pairwise
    formula, rank after rank, with the running mean carried as the first rank's shift plus an offset: delta = (c_r - c) + (off_r - off) is
    then a difference of small numbers -- formed from the rounded means c + off it would lose u |mean| and, far from the origin, the bound
    on sd^2 with it."""
    n = c0 = off = m2 = None
    for (nr, c, s1, s2) in parts:
        nr = np.asarray(nr, dtype=np.int64)
        c, s1, s2 = (np.asarray(a, dtype=np.float64) for a in (c, s1, s2))
        w = nr.astype(np.float64)
        has = nr > 0
        safe = np.where(has, w, 1.0)
        with np.errstate(over="ignore", invalid="ignore"):
            offr = np.where(has, s1 / safe, 0.0)
            m2r = np.where(has, s2 - s1 * s1 / safe, 0.0)
            if n is None:
                n, c0, off, m2 = nr.copy(), np.where(has, c, 0.0), offr, m2r
                continue
            tot = n + nr
            tw = np.where(tot > 0, tot.astype(np.float64), 1.0)
            first = has & (n == 0)
            c0 = np.where(first, c, c0)
            delta = np.where(has, (c - c0) + (offr - off), 0.0)
            off = np.where(first, offr, off + delta * (w / tw))
            m2 = np.where(first, m2r, m2 + m2r + delta * delta * (n.astype(np.float64) * w / tw))
        n = tot
    return n, c0 + off, m2


def finish(n, mean, m2, n_nan, n_pinf, n_ninf):
    """np.mean and np.std (ddof 0) of values of which n are finite (their pooled mean and M2), n_nan NaN, n_pinf +inf and n_ninf -inf"""
    n_nan, n_pinf, n_ninf = (np.asarray(a) > 0 for a in (n_nan, n_pinf, n_ninf))
    safe = np.where(n > 0, n.astype(np.float64), 1.0)
    mean = np.where(n > 0, mean, np.nan)
    mean = np.where(n_pinf, np.inf, mean)
    mean = np.where(n_ninf, -np.inf, mean)
    mean = np.where(n_nan | (n_pinf & n_ninf), np.nan, mean)
    sd = np.where(n > 0, np.sqrt(np.maximum(m2, 0.0) / safe), np.nan)
    sd = np.where(n_nan | n_pinf | n_ninf, np.nan, sd)
    return mean, sd


def pick_best(parts):
    """parts: per rank (best_ll, best_row, best_x), in rank order (row -1: the rank has no log-likelihood that is not NaN) -> the largest
    log-likelihood, the smallest row among equal ones, the first rank among equal rows"""
    best = None
    for (ll, row, x) in parts:
        ll, row = float(ll), int(row)
        if row < 0 or ll != ll:
            continue
        if best is None or ll > best[0] or (ll == best[0] and row < best[1]):
            best = (ll, row, np.array(x, dtype=np.float64))
    return best


def compute(trace_bins, trace_chains, allgather, n_burn, n_chains, history_rows, dim, every=1, chains=None):
    """The collective driver.  trace_bins(g0, g1, every) -> (counts (2, T, dim), sums (5, T, dim), ll_counts (4, T), ll_sums (5, T), best_ll,
    best_row, best_x) of this rank's chains, best_row an index of the super chain (HipEngine.trace_bins); trace_chains(chains) -> (pos, x
    (T, c, dim), ll (T, c)) for the c requested global chains this rank holds, pos their positions in the request (HipEngine.trace_chains);
    allgather(obj) -> [obj of every rank] in rank order ([obj] for one process, single_process_allgather).
    -> PosteriorTrace, the same bits on every rank"""
    n_burn = check_n_burn(WHO, n_burn)
    every = check_every(every)
    n_chains, dim = int(n_chains), int(dim)
    ch = check_chains(chains, n_chains)
    g0, g1 = window(n_burn, n_chains, history_rows)
    if g0 >= g1:
        trace_bins(g1, g1, every)      # (no generation: a sampler without a resident history says so here, in the library's words)
        raise empty_window(WHO, n_burn)
    every = min(every, g1 - g0)
    gen = np.arange(g0, g1, every, dtype=np.int64)
    T = len(gen)
    n = (np.minimum(gen + every, g1) - gen) * n_chains
    parts = allgather(trace_bins(g0, g1, every))
    counts = [np.asarray(p[0], dtype=np.int64).reshape(2, T, dim) for p in parts]
    sums = [np.asarray(p[1], dtype=np.float64).reshape(5, T, dim) for p in parts]
    ll_counts = [np.asarray(p[2], dtype=np.int64).reshape(4, T) for p in parts]
    ll_sums = [np.asarray(p[3], dtype=np.float64).reshape(5, T) for p in parts]

    def envelope(sm, n_not_nan):
        mn = np.min([s[3] for s in sm], axis=0)
        mx = np.max([s[4] for s in sm], axis=0)
        return np.where(n_not_nan > 0, mn, np.nan), np.where(n_not_nan > 0, mx, np.nan)

    n_nan = np.sum([c[1] for c in counts], axis=0)
    mn, mx = envelope(sums, n[:, None] - n_nan)
    nf, mean, m2 = merge_moments([(c[0], s[0], s[1], s[2]) for c, s in zip(counts, sums)])
    mean, sd = finish(nf, mean, m2, n_nan, mx == np.inf, mn == -np.inf)
    ll_nan = np.sum([c[1] for c in ll_counts], axis=0)
    ll_min, ll_max = envelope(ll_sums, n - ll_nan)
    nf, ll_mean, m2 = merge_moments([(c[0], s[0], s[1], s[2]) for c, s in zip(ll_counts, ll_sums)])
    ll_mean, _ = finish(nf, ll_mean, m2, ll_nan, np.sum([c[2] for c in ll_counts], axis=0), np.sum([c[3] for c in ll_counts], axis=0))
    best = pick_best([(p[4], p[5], p[6]) for p in parts])
    if best is None:
        best = (np.nan, -1, np.full(dim, np.nan))
    chain_x = np.full((T, len(ch), dim), np.nan)
    chain_ll = np.full((T, len(ch)), np.nan)
    if len(ch):
        seen = np.zeros(len(ch), dtype=np.int64)
        for (pos, x, ll) in allgather(trace_chains(ch)):
            pos = np.asarray(pos, dtype=np.int64).reshape(-1)
            if len(pos):
                chain_x[:, pos] = np.asarray(x, dtype=np.float64).reshape(T, len(pos), dim)
                chain_ll[:, pos] = np.asarray(ll, dtype=np.float64).reshape(T, len(pos))
                np.add.at(seen, pos, 1)
        if np.any(seen != 1):
            raise RuntimeError("%s: chains %s were returned by %s ranks (every chain has one owner)"
                               % (WHO, ch[seen != 1].tolist(), seen[seen != 1].tolist()))
    return PosteriorTrace(gen, n, mean, sd, mn, mx, n_nan, ll_mean, ll_min, ll_max, float(best[0]), best[2], int(best[1]), ch, chain_x, chain_ll)
