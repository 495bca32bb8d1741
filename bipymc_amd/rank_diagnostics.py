"""Rank-normalized convergence diagnostics of a sampler's resident history: the rank-normalized split-R-hat, bulk-ESS and tail-ESS of
Vehtari, Gelman, Simpson, Carpenter and Buerkner, "Rank-normalization, folding, and localization: an improved R-hat for assessing convergence
of MCMC", Bayesian Analysis 16 (2021) -- what Stan and ArviZ report.  The classic pair (diagnostics.py) is taken over moments of the raw
values: it misses chains that differ in scale but not in mean, is undefined for heavy tails and says nothing about how well the 5 % and 95 %
quantiles are estimated.

A ranked history is a history.  The GPU writes a transform of the window's split rows into the history of a second, ordinary handle
(bpm_rank_history, bipymc_amd/csrc/ranks.h); the split R-hat / ESS the project already has (diagnostics.compute over that handle's
bpm_diag_split_moments / bpm_diag_autocov) does the rest.  Four fills into one scratch handle, one after the other.

Definitions (per coordinate; the window of diagnostics.py: g0 = ceil(n_burn / n_chains), g1 = history rows, n = (g1 - g0) // 2; the split rows
are history rows [g0, g0 + n) then [g1 - n, g1) of every chain -- an odd window drops its middle row; S = 2 n n_chains values):
  r       the average rank (1-based, ties share the mean of their ranks; -0.0 and +0.0 are ties) of a value among the S values
  z       Phi^-1((r - 3/8) / (S + 1/4))
  bulk    z of x;    folded: z of |x - med|, med = np.median of the S values
  lower   1.0 where x <= q_lo, else 0.0;    upper: the same with q_hi;    q_lo, q_hi = np.quantile of the S values at prob
  r_hat_bulk, ess_bulk = r_hat, ess of bulk;  r_hat_tail = r_hat of folded;  r_hat = max(r_hat_bulk, r_hat_tail)
  ess_lower, ess_upper = ess of lower, upper;  ess_tail = min(ess_lower, ess_upper)
A coordinate whose window holds a NaN, or that is constant, has NaN in every one of these; +-inf are ordinary values for the ranks.
Single rank only: the pooled ranks of a history spread over several ranks are not built yet.
"""
from __future__ import division

import collections

import numpy as np

from . import diagnostics as _diag
from . import quantiles as _qs

KIND_RANK, KIND_Z, KIND_Z_FOLDED, KIND_INDICATOR, KIND_RANK_FOLDED, KIND_SQDEV = 0, 1, 2, 3, 4, 5      # (bipymc_amd/csrc/ranks.h)
DEFAULT_PROB = (0.05, 0.95)

RankDiagnostics = collections.namedtuple(
    "RankDiagnostics", ["r_hat", "r_hat_bulk", "r_hat_tail", "ess_bulk", "ess_tail", "ess_lower", "ess_upper", "median", "quantiles",
                        "ess_capped", "n_half_chains", "n_draws", "window"])
RankDiagnostics.__doc__ = """r_hat = max(r_hat_bulk, r_hat_tail), ess_bulk, ess_tail = min(ess_lower, ess_upper): (dim,) float64, NaN for a
coordinate that is constant or holds a NaN; median (dim,), quantiles (2, dim): np.median and np.quantile(prob) of the window's split rows;
ess_capped: (dim,) bool -- max_lag ended an autocorrelation sum of one of the four passes before Geyer's rule did; n_half_chains, n_draws: m
and n; window: (g0, g1), the history rows the split rows are taken from."""


def check_single_rank(who, n_ranks):
    if int(n_ranks) != 1:
        raise NotImplementedError("%s: pooled ranks are built on a single rank only (this communicator has %d ranks)" % (who, int(n_ranks)))


def check_prob(who, prob):
    """-> (lo, hi) floats with 0 < lo < hi < 1"""
    try:
        lo, hi = prob
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError("%s: prob must be a pair (lo, hi) of probabilities (got %r)" % (who, prob))
    if not 0.0 < lo < hi < 1.0:
        raise ValueError("%s: prob must satisfy 0 < lo < hi < 1 (got %r)" % (who, prob))
    return lo, hi


def median_positions(S):
    """0-based order statistics np.median of S values averages"""
    return ((S - 1) // 2, S // 2)


def summaries(S, q, positions, order_stats):
    """order_stats (len(positions), dim): those 0-based order statistics of every coordinate (NaN sorts last: position S - 1 must be among
    them) -> (median (dim,), np.quantile(q) (len(q), dim), has_nan (dim,) bool), as NumPy computes them"""
    at = {int(p): i for i, p in enumerate(positions)}
    os_ = np.asarray(order_stats, dtype=np.float64).reshape(len(positions), -1)
    has_nan = np.isnan(os_[at[S - 1]])
    a, b = median_positions(S)
    with np.errstate(invalid="ignore"):
        med = np.mean(np.stack([os_[at[a]], os_[at[b]]]), axis=0)
        quant = _qs.finish(S, np.asarray(q, dtype=np.float64), lambda rr: os_[[at[int(r)] for r in rr]], has_nan)
    return np.where(has_nan, np.nan, med), quant, has_nan


def positions_for(S, q):
    """the distinct order statistics median, np.quantile(q) and the NaN test need, sorted"""
    prev, nxt, _ = _qs.targets(S, np.asarray(q, dtype=np.float64))
    return np.unique(np.concatenate([prev.reshape(-1), nxt.reshape(-1), np.asarray(median_positions(S) + (S - 1,), dtype=np.int64)]))


def split_size(g0, g1, n_chains):
    """-> (n, S) of the window of history rows [g0, g1)"""
    n = (int(g1) - int(g0)) // 2
    return n, 2 * n * int(n_chains)


def compute(engine, allgather, g0, g1, max_lag=None, prob=DEFAULT_PROB, who="convergence_diagnostics_rank", keep_scratch=False):
    """The driver.  engine.rank_history(g0, g1, kind, arg, positions, dst) -> (dst, order_stats): HipEngine.rank_history -- dst (None: a new
    one) an engine with diag_split_moments, diag_autocov and close, whose history is the transformed split rows; allgather(obj) -> [obj] (one
    process).  Four fills into one dst, diagnostics.compute after each; dst is closed on every way out.  -> RankDiagnostics.
    keep_scratch=True: -> (RankDiagnostics, dst), dst still open for a further fill of the same window (summary.py's squared deviations) and
    the caller's to close; an error closes it as before."""
    lo, hi = check_prob(who, prob)
    g0, g1 = int(g0), int(g1)
    n, S = split_size(g0, g1, engine.n_chains)
    pos = positions_for(S, (lo, hi)) if n >= 4 else np.zeros(0, dtype=np.int64)      # (n < 4: the fill's own error)
    held = [None]                         # the scratch handle, from the moment the first fill returns it

    def fill(kind, arg=None, positions=()):
        held[0], os_ = engine.rank_history(g0, g1, kind, arg, positions, held[0])
        return os_, _diag.compute(held[0].diag_split_moments, held[0].diag_autocov, allgather, 0, 2 * n, max_lag=max_lag)

    try:
        os_, bulk = fill(KIND_Z, positions=pos)
        med, quant, _ = summaries(S, (lo, hi), pos, os_)
        folded = fill(KIND_Z_FOLDED, arg=med)[1]
        lower = fill(KIND_INDICATOR, arg=quant[0])[1]
        upper = fill(KIND_INDICATOR, arg=quant[1])[1]
    except BaseException:
        keep_scratch = False
        raise
    finally:
        if held[0] is not None and not keep_scratch:
            held[0].close()
    out = RankDiagnostics(
        r_hat=np.maximum(bulk.r_hat, folded.r_hat), r_hat_bulk=bulk.r_hat, r_hat_tail=folded.r_hat, ess_bulk=bulk.ess,
        ess_tail=np.minimum(lower.ess, upper.ess), ess_lower=lower.ess, ess_upper=upper.ess, median=med, quantiles=quant,
        ess_capped=bulk.ess_capped | folded.ess_capped | lower.ess_capped | upper.ess_capped, n_half_chains=bulk.n_half_chains,
        n_draws=bulk.n_draws, window=(g0, g1))
    return (out, held[0]) if keep_scratch else out


def ranked_engine(engine, g0, g1, scale="z", folded=False, who="rank_history"):
    """-> an engine whose history is the transformed split rows (the caller closes it): scale "z" the normal scores, "rank" the average
    ranks themselves; folded: of |x - median| instead of x"""
    if scale not in ("z", "rank"):
        raise ValueError("%s: scale must be 'z' or 'rank' (got %r)" % (who, scale))
    g0, g1 = int(g0), int(g1)
    if not folded:
        return engine.rank_history(g0, g1, KIND_Z if scale == "z" else KIND_RANK, None, (), None)[0]
    n, S = split_size(g0, g1, engine.n_chains)
    pos = np.unique(np.asarray(median_positions(S) + (S - 1,), dtype=np.int64)) if n >= 4 else np.zeros(0, dtype=np.int64)
    dst, os_ = engine.rank_history(g0, g1, KIND_RANK, None, pos, None)
    try:
        med = summaries(S, (0.5,), pos, os_)[0]
        return engine.rank_history(g0, g1, KIND_Z_FOLDED if scale == "z" else KIND_RANK_FOLDED, med, (), dst)[0]
    except BaseException:
        dst.close()
        raise
