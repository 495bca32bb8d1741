"""The posterior summary table of a sampler's resident history -- what Stan, ArviZ and the `posterior` package print per parameter: mean, sd,
a highest-density interval, the Monte Carlo standard errors of mean and sd, the effective sample sizes and R-hat -- taken where the history
lies.  The GPU sorts the columns and scans them (bpm_hdi, bipymc_amd/csrc/ranks.h: rk_hdi_kernel) and writes the squared deviations into the
scratch handle of the rank diagnostics (bpm_rank_history kind 5); the split R-hat / ESS the project already has (diagnostics.py,
rank_diagnostics.py) does the rest on arrays of a few times `dim` values.

Definitions (per coordinate, over the S values of the window):
  HDI of probability p, 0 < p < 1:   s = sort(values);  m = min(floor(p * S), S - 1);  w[i] = s[i + m] - s[i], i in [0, S - m);
      i* = the first i whose w[i] is NaN (inf - inf) if any is, else the first i of the smallest w (np.argmin's rule);  (s[i*], s[i* + m]).
      A coordinate whose window holds a NaN has (NaN, NaN); -0.0 and +0.0 are one value.
  mean, sd       the mean and np.std(ddof=1) of the values, from the split-chain moments (half-chain means and variances of equal length n:
                 mean = mean of the half-chain means, (S - 1) sd^2 = (n - 1) sum_j s2_j + n sum_j (xbar_j - mean)^2); a coordinate with
                 a NaN or an inf among the values has mean = sd = NaN, as all its split-chain moments are (np.mean's +-inf is not restored)
  mcse_mean      sd / sqrt(ess_mean),  ess_mean the classic ESS of the values (diagnostics.py)
  ess_sd         the classic ESS of d = (x - mean)^2
  mcse_sd        sqrt(((mean(d^2) - mean(d)^2) / ess_sd) / mean(d) / 4): the delta method on sqrt(mean(d)) -- sd / sqrt(2 S) for independent
                 Gaussian draws.  mean(d) and mean(d^2) - mean(d)^2 come from the shifted sums of bpm_reduce_moments over the scratch handle.
param_est_hdi's window is param_est's: the super-chain rows >= n_burn.  posterior_summary's is the split rows of convergence_diagnostics'
window (diagnostics.py: g0 = ceil(n_burn / n_chains), the first and the last n = (g1 - g0) // 2 history rows of every chain), so that every
column of the table speaks of the same S = 2 n n_chains draws.  Single rank only, like the pooled ranks.
"""
from __future__ import division

import collections
import math

import numpy as np

from . import diagnostics as _diag
from . import rank_diagnostics as _rk

MAX_PROB = 8                      # probabilities of one bpm_hdi call (bipymc_amd/csrc/ranks.h: RK_MAX_PROB)
WINDOW_SPLIT_ROWS, WINDOW_PARAM_EST = 0, 1
DEFAULT_HDI_PROB = 0.94

PosteriorHDI = collections.namedtuple("PosteriorHDI", ["lo", "hi", "prob", "n_nan", "n"])
PosteriorHDI.__doc__ = """lo, hi: (dim,) float64 for a scalar prob, (len(prob), dim) for a sequence -- the highest-density interval of every
coordinate, (NaN, NaN) where the window holds a NaN; prob: as given; n_nan: (dim,) int64 NaNs per coordinate; n: values per coordinate."""

_FIELDS = ["mean", "sd", "hdi_lo", "hdi_hi", "hdi_prob", "median", "quantiles", "prob", "mcse_mean", "mcse_sd", "ess_mean", "ess_sd",
           "ess_bulk", "ess_tail", "r_hat", "r_hat_classic", "ess_capped", "n_nan", "n_half_chains", "n_draws", "window", "rank"]


class PosteriorSummary(collections.namedtuple("PosteriorSummary", _FIELDS)):
    """mean, sd, hdi_lo, hdi_hi, median, mcse_mean, mcse_sd, ess_mean, ess_sd, ess_bulk, ess_tail, r_hat (rank-normalized), r_hat_classic:
    (dim,) float64; quantiles: (2, dim), np.quantile(prob); ess_capped: (dim,) bool -- max_lag ended an autocorrelation sum of one of the
    six passes before Geyer's rule did; n_nan: (dim,) int64; hdi_prob, prob: as given; n_half_chains, n_draws: m and n, S = m n values per
    coordinate; window: (g0, g1), the history rows the split rows are taken from; rank: the whole rank_diagnostics.RankDiagnostics (r_hat_bulk,
    r_hat_tail, ess_lower, ess_upper) the rank columns are taken from.  str() is the table, one line per coordinate."""
    __slots__ = ()

    def __str__(self):
        names = ["mean", "sd", "hdi_%g%%" % (50.0 * (1.0 - self.hdi_prob)), "hdi_%g%%" % (50.0 * (1.0 + self.hdi_prob)), "mcse_mean", "mcse_sd",
                 "ess_bulk", "ess_tail", "r_hat"]
        cols = [self.mean, self.sd, self.hdi_lo, self.hdi_hi, self.mcse_mean, self.mcse_sd, self.ess_bulk, self.ess_tail, self.r_hat]
        lines = ["%-6s" % "coord" + "".join("%12s" % n for n in names)]
        for k in range(len(self.mean)):
            lines.append("%-6d" % k + "".join("%12.5g" % float(c[k]) for c in cols))
        lines.append("%d draws per coordinate: %d half-chains of %d, history rows [%d, %d)"
                     % (self.n_half_chains * self.n_draws, self.n_half_chains, self.n_draws, self.window[0], self.window[1]))
        return "\n".join(lines)


def check_hdi_prob(who, prob):
    """-> (probabilities as a float64 vector, whether prob was a scalar); 1 ... MAX_PROB of them, each inside (0, 1)"""
    scalar = np.ndim(prob) == 0
    try:
        p = np.asarray(prob, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("%s: prob must be a probability or a sequence of probabilities (got %r)" % (who, prob))
    if not 1 <= len(p) <= MAX_PROB:
        raise ValueError("%s: %d probabilities given; one call takes 1 ... %d" % (who, len(p), MAX_PROB))
    for x in p:
        if not 0.0 < x < 1.0:
            raise ValueError("%s: every probability must lie inside (0, 1) (got %r)" % (who, float(x)))
    return p, scalar


def hdi_offset(p, S):
    """m = min(floor(p * S), S - 1), in the double arithmetic bpm_hdi uses"""
    return min(int(math.floor(float(p) * float(int(S)))), int(S) - 1)


def sd_of_split_moments(m, n, m2_of_means, sum_of_vars):
    """np.std(ddof=1) of the m n pooled values of m half-chains of n draws from their moments: the sum of squares about the pooled mean is
    the sum within the half-chains, (n - 1) sum_j s2_j, plus the sum between them, n sum_j (xbar_j - mean)^2"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(((n - 1.0) * np.asarray(sum_of_vars) + float(n) * np.asarray(m2_of_means)) / (m * n - 1.0))


def mcse_of_sd(mean_d, var_d, ess_sd):
    """sqrt((var(d) / ess_sd) / mean(d) / 4), d = (x - mean)^2 with var(d) = mean(d^2) - mean(d)^2"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(((var_d / ess_sd) / mean_d) / 4.0)


def shifted_mean_var(count, s1, s2, shift):
    """count, sum (x - shift), sum (x - shift)^2, shift (HipEngine.reduce_moments) -> (mean, mean(x^2) - mean(x)^2)"""
    n = float(count)
    with np.errstate(invalid="ignore"):
        return shift + s1 / n, s2 / n - (s1 / n) ** 2


def compute_hdi(engine, n_burn, prob, n_chains, who="param_est_hdi"):
    """param_est_hdi's driver.  engine.hdi(window, a, b, prob) -> (lo, hi, n_nan, S, _): HipEngine.hdi.  -> PosteriorHDI"""
    from ._history_stats import check_n_burn, empty_window
    n_burn = check_n_burn(who, n_burn)
    p, scalar = check_hdi_prob(who, prob)
    rows = engine.history_rows()
    if rows > 0 and rows * int(n_chains) - n_burn <= 0:
        raise empty_window(who, n_burn)
    lo, hi, n_nan, S, _ = engine.hdi(WINDOW_PARAM_EST, n_burn, 0, p)
    return PosteriorHDI(lo=lo[0] if scalar else lo, hi=hi[0] if scalar else hi, prob=prob, n_nan=n_nan, n=S)


def compute(engine, allgather, g0, g1, hdi_prob=DEFAULT_HDI_PROB, prob=_rk.DEFAULT_PROB, max_lag=None, who="posterior_summary"):
    """posterior_summary's driver over the split rows of history rows [g0, g1).  engine: a HipEngine (diag_split_moments, diag_autocov,
    rank_history, hdi); allgather(obj) -> [obj] (one process).  The rank diagnostics' scratch handle takes a fifth fill, the squared
    deviations, and is closed on every way out.  -> PosteriorSummary"""
    p, scalar = check_hdi_prob(who, hdi_prob)
    if not scalar:
        raise ValueError("%s: hdi_prob must be one probability (param_est_hdi takes several)" % who)
    _rk.check_prob(who, prob)
    g0, g1 = int(g0), int(g1)
    seen = {}

    def split_moments(a, b):
        seen["parts"] = engine.diag_split_moments(a, b)
        return seen["parts"]

    classic = _diag.compute(split_moments, engine.diag_autocov, allgather, g0, g1, max_lag=max_lag)
    m, n, mean, m2, sv = _diag.merge_split_moments(allgather(seen["parts"]))
    sd = sd_of_split_moments(m, n, m2, sv)
    lo, hi, n_nan, S, _ = engine.hdi(WINDOW_SPLIT_ROWS, g0, g1, p)
    rank, dst = _rk.compute(engine, allgather, g0, g1, max_lag=max_lag, prob=prob, who=who, keep_scratch=True)
    try:
        engine.rank_history(g0, g1, _rk.KIND_SQDEV, mean, (), dst)
        dev = _diag.compute(dst.diag_split_moments, dst.diag_autocov, allgather, 0, 2 * n, max_lag=max_lag)
        mean_d, var_d = shifted_mean_var(*dst.reduce_moments(0))
    finally:
        dst.close()
    with np.errstate(invalid="ignore", divide="ignore"):
        mcse_mean = sd / np.sqrt(classic.ess)
    return PosteriorSummary(
        mean=mean, sd=sd, hdi_lo=lo[0], hdi_hi=hi[0], hdi_prob=float(p[0]), median=rank.median, quantiles=rank.quantiles,
        prob=tuple(float(x) for x in prob), mcse_mean=mcse_mean, mcse_sd=mcse_of_sd(mean_d, var_d, dev.ess), ess_mean=classic.ess,
        ess_sd=dev.ess, ess_bulk=rank.ess_bulk, ess_tail=rank.ess_tail, r_hat=rank.r_hat, r_hat_classic=classic.r_hat,
        ess_capped=classic.ess_capped | rank.ess_capped | dev.ess_capped, n_nan=n_nan, n_half_chains=int(m), n_draws=int(n), window=(g0, g1),
        rank=rank)
