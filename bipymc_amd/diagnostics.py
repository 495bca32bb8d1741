"""Convergence diagnostics of a sampler's resident history: split-chain R-hat and the effective sample size (ESS).

The GPU reduces the history (bpm_diag_split_moments / bpm_diag_autocov, bipymc_amd/csrc/diagnostics.h); this module combines the
per-rank parts and finishes the statistics on arrays of a few times `dim` values.  Every rank of a world runs the same arithmetic on the
same gathered parts in the same order, so every rank returns the same bits.

Definitions (per coordinate, window of history rows [g0, g1), g0 = ceil(n_burn / n_chains), row 0 = the initial state):
  n = floor((g1 - g0) / 2) draws per half-chain; every chain gives the half-chains [g0, g0 + n) and [g1 - n, g1) (an odd window drops its
  middle row); m = 2 n_chains half-chains; n < 4 is an error.
  xbar_j, s2_j (ddof 1) and c_{j,t} = (1/n) sum_{i=0}^{n-1-t} (x_{j,i} - xbar_j)(x_{j,i+t} - xbar_j) of half-chain j;
  W = mean_j s2_j,  B/n = var_j(xbar_j, ddof 1),  var+ = (n - 1)/n W + B/n,  r_hat = sqrt(var+ / W);
  C_t = mean_j c_{j,t},  rho_t = 1 - (W - C_t) / var+  (rho_0 := 1);
  Geyer's initial positive sequence, then his initial monotone sequence (the procedure of Stan and of ArviZ's ess(method="mean") on split
  chains), written out in geyer() below;  tau = max(-1 + 2 sum_{t <= max_t} rho_t (+ rho_{max_t + 1} if kept), 1 / log10(m n));
  ess = m n / tau.
  W == 0 (a coordinate constant in every half-chain): r_hat = ess = tau = NaN.
  A coordinate with a NaN or +-inf in either half: every part the device returns for it is NaN (the mean of the means too, whatever the
  sign of an inf), so r_hat = ess = tau = NaN; the other coordinates are what they would be without that value, bit for bit.
"""
from __future__ import division

import collections
import math

import numpy as np

from .comm import single_process_allgather  # noqa: F401  (for callers without a communicator)

ConvergenceDiagnostics = collections.namedtuple(
    "ConvergenceDiagnostics", ["r_hat", "ess", "tau", "ess_capped", "lags_used", "n_half_chains", "n_draws", "window"])
ConvergenceDiagnostics.__doc__ = """r_hat, ess, tau: (dim,) float64; ess_capped: (dim,) bool -- max_lag ended the autocorrelation sum before Geyer's
rule did; lags_used: (dim,) int -- autocorrelation lags the truncation read (0 ... lags_used - 1); n_half_chains, n_draws: m and n;
window: (g0, g1), the history rows the statistics are taken over."""

# lags requested from the device per call: the autocovariance kernel's block (diagnostics.h: DIAG_T)
LAG_BLOCK = 16


def window(n_burn, n_chains, history_rows):
    """(g0, g1): n_burn in super-chain rows (param_est's unit: row g * n_chains + i = chain i at generation g) -> the first whole generation"""
    n_burn = max(0, int(n_burn))
    return -(-n_burn // int(n_chains)), int(history_rows)


def merge_split_moments(parts):
    """parts: per rank (mean_of_means, m2_of_means, sum_of_vars, n_half_chains, n_draws), in rank order -> (m, n, mean, m2, sum_of_vars).
    The means and their sums of squared deviations combine with Chan et al.'s pairwise formula, the variances add."""
    mean, m2, sv, m, n = None, None, None, 0, None
    for (pm, pm2, psv, pm_half, pn) in parts:
        pm, pm2, psv = np.asarray(pm, dtype=np.float64), np.asarray(pm2, dtype=np.float64), np.asarray(psv, dtype=np.float64)
        if n is not None and int(pn) != n:
            raise ValueError("ranks disagree on the window (%d != %d draws per half-chain)" % (int(pn), n))
        n = int(pn)
        if m == 0:
            mean, m2, sv, m = pm.copy(), pm2.copy(), psv.copy(), int(pm_half)
            continue
        mb = int(pm_half)
        delta = pm - mean
        tot = m + mb
        mean = mean + delta * (mb / tot)
        m2 = m2 + pm2 + delta * delta * (m * mb / tot)
        sv = sv + psv
        m = tot
    return m, n, mean, m2, sv


def r_hat_terms(m, n, m2_of_means, sum_of_vars):
    """-> (W, var_plus, r_hat); r_hat is NaN where W == 0"""
    W = sum_of_vars / m
    var_plus = (n - 1.0) / n * W + m2_of_means / (m - 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_hat = np.sqrt(var_plus / W)
    r_hat = np.where(W > 0, r_hat, np.nan)
    return W, var_plus, r_hat


def autocorrelation(c_sum, m, W, var_plus):
    """c_sum: (lags, dim) sums over all half-chains of c_{j,t} -> rho_t (lags, dim), rho_0 = 1"""
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = 1.0 - (W[None, :] - c_sum / m) / var_plus[None, :]
    if rho.shape[0]:
        rho[0, :] = 1.0
    return rho


def geyer(rho, n, m, top):
    """Geyer's initial positive + initial monotone sequence on rho[0 ... len(rho) - 1] (rho[0] is taken as 1) of half-chains of n draws.
    top: the largest lag that may be read (max_lag, at most n - 1).
    -> (tau, lags_used, capped), or None when the next lag is needed: len(rho) <= top and the sequence has not ended."""
    avail = len(rho)
    if avail < 2:
        return None if top >= 1 else (float("nan"), 0, True)
    rt = [1.0, float(rho[1])]                  # rho_hat_t[0 ... t]
    even, odd = 1.0, float(rho[1])
    t = 1
    capped = False
    # 1./2. pairs (rho_{t+1}, rho_{t+2}), t = 1, 3, ...: kept while t < n - 3 and the previous pair's sum is > 0, stored if their sum is >= 0
    while t < n - 3 and even + odd > 0.0:
        if t + 2 > top:
            capped = True
            break
        if t + 2 >= avail:
            return None
        even, odd = float(rho[t + 1]), float(rho[t + 2])
        if even + odd >= 0.0:
            rt += [even, odd]
        else:
            rt += [0.0, 0.0]
        t += 2
    max_t = t - 2
    # 3. the last even value, if positive
    if even > 0.0:
        rt[max_t + 1] = even
    # 4. initial monotone sequence: pair sums made non-increasing by averaging
    t = 1
    while t <= max_t - 2:
        if rt[t + 1] + rt[t + 2] > rt[t - 1] + rt[t]:
            rt[t + 1] = (rt[t - 1] + rt[t]) / 2.0
            rt[t + 2] = rt[t + 1]
        t += 2
    r = np.asarray(rt, dtype=np.float64)
    tau = -1.0 + 2.0 * np.sum(r[:max_t + 1]) + np.sum(r[max_t + 1:max_t + 2])
    tau = max(tau, 1.0 / math.log10(m * n))
    if np.isnan(r).any():
        tau = float("nan")
    return float(tau), max_t + 3, capped


def compute(split_moments, autocov, allgather, g0, g1, max_lag=None, block=LAG_BLOCK):
    """The collective driver.  split_moments(g0, g1) / autocov(t0, n_lags): this rank's parts (HipEngine.diag_split_moments /
    diag_autocov); allgather(obj) -> [obj of every rank] in rank order (a communicator's allgather; [obj] for one process).  Lags are
    requested `block` at a time until every coordinate's sequence has ended or max_lag is reached."""
    m, n, _mean, m2, sv = merge_split_moments(allgather(split_moments(int(g0), int(g1))))
    W, var_plus, r_hat = r_hat_terms(m, n, m2, sv)
    d = len(W)
    if max_lag is not None and int(max_lag) < 1:
        raise ValueError("max_lag must be >= 1")
    top = n - 1 if max_lag is None else min(int(max_lag), n - 1)
    live = [k for k in range(d) if W[k] > 0 and np.isfinite(var_plus[k])]
    done = {}
    c_sum = np.zeros((0, d))
    while True:
        rho = autocorrelation(c_sum, m, W, var_plus)
        for k in live:
            if k not in done:
                r = geyer(rho[:, k], n, m, top)
                if r is not None:
                    done[k] = r
        if len(done) == len(live):
            break
        t0 = c_sum.shape[0]
        parts = allgather(autocov(t0, min(int(block), top + 1 - t0)))
        tot = np.array(parts[0], dtype=np.float64)
        for p in parts[1:]:
            tot = tot + p
        c_sum = np.concatenate([c_sum, tot], axis=0)
    tau = np.full(d, np.nan)
    lags = np.zeros(d, dtype=np.int64)
    capped = np.zeros(d, dtype=bool)
    for k, (tk, lk, ck) in done.items():
        tau[k], lags[k], capped[k] = tk, lk, ck
    ess = (m * n) / tau
    return ConvergenceDiagnostics(r_hat=r_hat, ess=ess, tau=tau, ess_capped=capped, lags_used=lags, n_half_chains=int(m), n_draws=int(n),
                                  window=(int(g0), int(g1)))
