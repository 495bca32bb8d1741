"""Model comparison where the history lives: WAIC and the pointwise expected log predictive density per datum (Watanabe 2010; Vehtari,
Gelman and Gabry 2017; what ArviZ's `waic` / `compare` report).

The fitting scripts of the reference sum a log density over their data points inside ln_like_fn (examples/ex_line_fit.py:63-67); which of
two such models predicts the data better is a statement about every single term of that sum over every draw of the posterior: with
l_is = the log density of datum i under draw s,

    lppd_i   = log mean_s exp(l_is)         p_waic_i = var_s(l_is)         elpd_i = lppd_i - p_waic_i.

That is an S x n_data matrix nobody can materialise (6e6 draws x 1e4 data points: 480 GB).  Here the density of ONE datum is a few lines of HIP,

    pw = HipPointwise('''
        __device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p) {
            const double r = y[1] - (x[0] + x[1] * y[0]);          // y: the w values of datum i
            return -0.5 * (r * r * p[0] - log(p[0]) + 1.8378770664093453);
        }''', data=np.column_stack([t, y]), params=[inv_sigma2])
    w = sampler.param_est_waic(pw, n_burn=N * 500)        # -> PosteriorWaic; str(w) is a short table
    elpd_diff, se_diff = compare_waic(w_a, w_b)

and the library compiles a streaming reduction around it whose parallel axis is the data (bipymc_amd/csrc/pointwise.h, pointwise_rows.h): a thread
per datum keeps an online log-sum-exp and the shifted moments of its l_is in registers while the rows of the window pass by.  x is one
super-chain row (d coordinates), y the w values of datum i, p the parameter block; the device math functions, INFINITY, NAN and M_PI are
there as for HipLikelihood, and the source is compiled -O3 -ffp-contract=off, so a formula of + - * / gives the bits NumPy gives.  The
pointwise density is independent of how the sampler's likelihood was given.

What the function must return: the log density of ONE datum, normalising constants included wherever two models with different noise
parameters are to be compared.

What is not finite follows NumPy / SciPy per datum and never crosses to another datum: some l_is = -inf leave lppd_i finite (p_waic_i is
NaN and mean_i -inf, as np.var and np.mean say); all -inf give lppd_i = -inf; any +inf gives +inf; any NaN gives NaN in lppd_i, p_waic_i and
mean_i.  The totals are plain np.sum of the per-datum arrays.  n_high_var counts the data with p_waic_i > 0.4, the condition under which
ArviZ warns that WAIC is unreliable and recommends PSIS-LOO: param_est_loo below.

PSIS-LOO (Vehtari, Simpson, Gelman, Yao and Gabry, "Pareto smoothed importance sampling"; Vehtari, Gelman and Gabry 2017; what ArviZ's `loo`
reports).  Leaving datum i out re-weights draw s by exp(-l_is); the largest of those ratios are replaced by quantiles of a generalised Pareto
distribution fitted to them, whose shape pareto_k says whether the estimate can be trusted (k > 0.7: it cannot -- the datum is an outlier or
has leverage).  Per datum, over the S draws of the window:

    M = ceil(min(S / 5, 3 sqrt(S / r_eff_i)));  the kept set: the K = min(M + 1, S) smallest l;  the cutoff c: its largest;  the tail: the kept
    values < c (ties with the cutoff belong to the body, so tail_len <= M);  tail_len <= 4: pareto_k = +inf, nothing is smoothed;  else the
    fit of Zhang and Stephens with ArviZ's prior, and if k is finite the tail's log weights become log(gpinv((j - 0.5) / n, k, sigma) +
    exp(-c - x_max)), truncated at 0;  elpd_loo_i = logsumexp(l + lw) - logsumexp(lw).

    loo = sampler.param_est_loo(pw, n_burn=N * 500)        # -> PosteriorLoo; str(loo) is a short table
    elpd_diff, se_diff = compare_loo(loo_a, loo_b)

Nothing of size S x n_data exists anywhere: a thread per datum selects its kept set exactly while the rows stream by (csrc/pointwise_tail.h),
a second pass takes the log-sum-exp of the rest, and a workgroup per datum fits and finishes (csrc/psis.h).  A datum with a value that is not
finite gets NaN in pareto_k, elpd_loo_i and p_loo_i and tail_len 0; its lppd_i and the counters are param_est_waic's.  Single rank only.

This module validates, merges the ranks in rank order -- the log-sum-exp by M = max(m_a, m_b), s = s_a exp(m_a - M) + s_b exp(m_b - M), the
moments by traces.merge_moments, the formulas of the device's own fold -- and finishes.  Every rank runs the same arithmetic on the same
gathered parts: every rank returns the same bits.
"""
from __future__ import division

import collections

import numpy as np

from ._history_stats import check_n_burn, empty_window
from .comm import single_process_allgather  # noqa: F401  (for callers without a communicator)
from .derived import gather_window
from .traces import finish, merge_moments

WHO = "param_est_waic"
WHO_LOO = "param_est_loo"
BAD_K = 0.7
MAX_DATA_W = 64
HIGH_VAR = 0.4
SIGNATURE = "__device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p)"


class PosteriorWaic(collections.namedtuple("PosteriorWaic", [
        "lppd_i", "p_waic_i", "elpd_i", "mean_i", "n_nan", "n_neg_inf", "n_pos_inf", "elpd_waic", "p_waic", "lppd", "se", "waic",
        "n_high_var", "n", "values"])):
    """Per datum, (n_data,): lppd_i = logsumexp_s(l_is) - log(n); p_waic_i = np.var(l_is, axis=0) (ddof 0); elpd_i = lppd_i - p_waic_i;
    mean_i = np.mean(l_is, axis=0); n_nan, n_neg_inf, n_pos_inf int64: how many l_is are NaN, -inf, +inf.  Totals: elpd_waic, p_waic, lppd
    = np.sum of those arrays; se = sqrt(n_data * np.var(elpd_i)); waic = -2 elpd_waic; n_high_var = how many p_waic_i exceed 0.4 (ArviZ
    warns then); n: rows of the window, summed over ranks; values: None, or the (n, n_data) matrix l_is in super-chain order"""
    __slots__ = ()

    def __str__(self):
        bad = [("NaN", self.n_nan), ("-inf", self.n_neg_inf), ("+inf", self.n_pos_inf)]
        rows = [("elpd_waic", "%.6g" % self.elpd_waic), ("se", "%.6g" % self.se), ("p_waic", "%.6g" % self.p_waic), ("lppd", "%.6g" % self.lppd),
                ("waic", "%.6g" % self.waic), ("n (draws)", "%d" % self.n), ("n_data", "%d" % len(self.lppd_i)),
                ("data with p_waic_i > %.1f" % HIGH_VAR, "%d" % self.n_high_var)]
        rows += [("data with a %s value" % name, "%d" % int(np.count_nonzero(c))) for name, c in bad]
        width = max(len(k) for k, _ in rows)
        return "\n".join("%-*s  %s" % (width, k, v) for k, v in rows)


class HipPointwise(object):
    """The log density of one datum as HIP source: `source` defines

        __device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p)      // y: the w values of datum i

    data: float64, (n_data, w) or (n_data,), 1 <= w <= 64, 1 <= n_data < 2^31 (HipLikelihood's rules), copied to the device once per
    sampler; params: the float64 block `p`.  python_fn(X (n, d), data, params) -> (n, n_data) (optional): the same statement for the host
    -- engines that cannot compile (CPU tests) use it."""

    def __init__(self, source, data, params=(), python_fn=None):
        arr = np.asarray(data)
        if arr.dtype != np.float64:
            raise ValueError("data must be float64 (got %s)" % arr.dtype)
        if arr.ndim == 1:
            arr = arr.reshape(-1, 1)
        if arr.ndim != 2:
            raise ValueError("data must have shape (n_data, w) or (n_data,) (got %r)" % (arr.shape,))
        if not 1 <= arr.shape[0] < 2 ** 31:
            raise ValueError("data must have 1 <= n_data < 2^31 rows (got %d)" % arr.shape[0])
        if not 1 <= arr.shape[1] <= MAX_DATA_W:
            raise ValueError("data must have 1 <= w <= %d values per datum (got %d)" % (MAX_DATA_W, arr.shape[1]))
        self.source = str(source)
        self.data = np.ascontiguousarray(arr)
        self.n_data, self.w = int(arr.shape[0]), int(arr.shape[1])
        self.params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        self.python_fn = python_fn

    def __call__(self, X):
        """the host statement on rows X (n, d) -> (n, n_data)"""
        if self.python_fn is None:
            raise TypeError("this HipPointwise has no python_fn: it can only be evaluated on the device")
        X = np.asarray(X, dtype=np.float64)
        out = np.asarray(self.python_fn(X, self.data, self.params), dtype=np.float64)
        if out.shape != (len(X), self.n_data):
            raise ValueError("HipPointwise: python_fn returned shape %r for %d rows and %d data points" % (out.shape, len(X), self.n_data))
        return out

    def check(self, arch=None):
        """Compile only (no GPU needed): raises ValueError with the compiler's log when the source does not build for `arch` (default gfx950)."""
        from ._lib import check_source
        return check_source("bpm_check_pointwise", self.source.encode(), self.w, arch=arch)


def merge_lse(parts):
    """parts: (n, m, s) arrays of one shape, in order: n finite values whose log-sum-exp is m + log(s), m their maximum (n = 0: nothing, m
    and s are not read) -> (n int64, m, s) of all of them (m = -inf, s = 0 where there is none).  The device's fold (csrc/pointwise.h:
    pw_merge_lse), restated: M = max(m_a, m_b), s = s_a exp(m_a - M) + s_b exp(m_b - M), formed only where both sides hold a value -- an
    empty side never meets an exp, so no inf - inf is formed."""
    n = m = s = None
    for (nb, mb, sb) in parts:
        nb = np.asarray(nb, dtype=np.int64)
        hb = nb > 0
        mb = np.where(hb, np.asarray(mb, dtype=np.float64), -np.inf)
        sb = np.where(hb, np.asarray(sb, dtype=np.float64), 0.0)
        if n is None:
            n, m, s = nb.copy(), mb, sb
            continue
        both = (n > 0) & hb
        M = np.maximum(m, mb)
        Mb = np.where(both, M, 0.0)
        ea = np.exp(np.where(both, m, 0.0) - Mb)
        eb = np.exp(np.where(both, mb, 0.0) - Mb)
        s = np.where(both, s * ea + sb * eb, np.where(hb, sb, s))
        m = M
        n = n + nb
    return n, m, s


def finish_waic(counts, m, s, mean, m2, n, vals=None):
    """counts (4, n_data) int64: finite | NaN | +inf | -inf values per datum; (m, s): the log-sum-exp of the finite ones; mean, m2: their
    pooled mean and sum of squared deviations; n: rows of the window -> PosteriorWaic"""
    n_fin, n_nan, n_pinf, n_ninf = (np.asarray(c, dtype=np.int64) for c in counts)
    some = n_fin > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        lppd_i = np.where(some, (m + np.log(np.where(some, s, 1.0))) - np.log(float(n)), -np.inf)
    lppd_i = np.where(n_pinf > 0, np.inf, lppd_i)
    lppd_i = np.where(n_nan > 0, np.nan, lppd_i)
    mean_i, _ = finish(n_fin, mean, m2, n_nan, n_pinf, n_ninf)
    all_finite = (n_nan + n_pinf + n_ninf) == 0
    p_waic_i = np.where(all_finite & some, np.maximum(m2, 0.0) / np.where(some, n_fin.astype(np.float64), 1.0), np.nan)
    with np.errstate(invalid="ignore"):
        elpd_i = lppd_i - p_waic_i
        elpd, p_waic, lppd = np.sum(elpd_i), np.sum(p_waic_i), np.sum(lppd_i)
        se = np.sqrt(len(elpd_i) * np.var(elpd_i))
        high = int(np.count_nonzero(p_waic_i > HIGH_VAR))
    return PosteriorWaic(lppd_i, p_waic_i, elpd_i, mean_i, n_nan, n_ninf, n_pinf, float(elpd), float(p_waic), float(lppd), float(se),
                         float(-2.0 * elpd), high, int(n), vals)


def compute(pointwise, allgather, pw, n_burn, n_chains, history_rows, values=False):
    """The collective driver.  pointwise(pw, n_burn, values) -> (counts (4, n_data) int64: finite | NaN | +inf | -inf, sums (5, n_data):
    shift | S1 | S2 | m | s, n_rows, n_first, values (n_rows, n_data) or None) of this rank's rows (HipEngine.pointwise); allgather(obj) ->
    [obj of every rank] in rank order ([obj] for one process, single_process_allgather).  -> PosteriorWaic, the same bits on every rank"""
    if not isinstance(pw, HipPointwise):
        raise TypeError("%s: pw must be a HipPointwise (got %s)" % (WHO, type(pw).__name__))
    n_burn = check_n_burn(WHO, n_burn)
    counts, sums, n, vals = gather_window(WHO, allgather, pointwise(pw, n_burn, bool(values)), n_burn, n_chains, history_rows, 4, pw.n_data, values)
    _, m, s = merge_lse([(c[0], sm[3], sm[4]) for c, sm in zip(counts, sums)])
    nf, mean, m2 = merge_moments([(c[0], sm[0], sm[1], sm[2]) for c, sm in zip(counts, sums)])
    total = np.sum(counts, axis=0)
    return finish_waic((nf, total[1], total[2], total[3]), m, s, mean, m2, n, vals)


def compare_waic(a, b):
    """-> (elpd_diff, se_diff) of two PosteriorWaic over the same data and as many draws: elpd_diff = a.elpd_waic - b.elpd_waic (positive:
    a predicts better), se_diff = sqrt(n_data * np.var(a.elpd_i - b.elpd_i)), the standard error of that difference (Vehtari, Gelman and
    Gabry 2017, eq. 24).  Host arithmetic only."""
    for x in (a, b):
        if not isinstance(x, PosteriorWaic):
            raise TypeError("compare_waic: both arguments must be PosteriorWaic (got %s)" % type(x).__name__)
    if len(a.elpd_i) != len(b.elpd_i):
        raise ValueError("compare_waic: the results are over %d and %d data points; both must be over the same data" % (len(a.elpd_i), len(b.elpd_i)))
    if a.n != b.n or a.n <= 0:
        raise ValueError("compare_waic: the results are over %d and %d draws; both must be over the same number, more than 0" % (a.n, b.n))
    with np.errstate(invalid="ignore"):
        diff = a.elpd_i - b.elpd_i
        return float(a.elpd_waic - b.elpd_waic), float(np.sqrt(len(diff) * np.var(diff)))


class PosteriorLoo(collections.namedtuple("PosteriorLoo", [
        "elpd_loo_i", "pareto_k", "lppd_i", "p_loo_i", "tail_len", "n_nan", "n_neg_inf", "n_pos_inf", "elpd_loo", "p_loo", "lppd", "se", "looic",
        "n_bad_k", "n", "tails", "stats"])):
    """Per datum, (n_data,): elpd_loo_i = logsumexp_s(l_is + lw_is) - logsumexp_s(lw_is) with lw the Pareto smoothed log weights; pareto_k:
    the fitted shape (+inf: a tail of 4 or fewer draws, nothing smoothed); lppd_i: param_est_waic's, the same bits; p_loo_i = lppd_i -
    elpd_loo_i; tail_len int64: how many draws were smoothed; n_nan, n_neg_inf, n_pos_inf int64.  Totals: elpd_loo, p_loo, lppd = np.sum of
    those arrays; se = sqrt(n_data * np.var(elpd_loo_i)); looic = -2 elpd_loo; n_bad_k = how many pareto_k exceed 0.7; n: rows of the window;
    tails: None, or a list of each datum's kept values (its K smallest l), ascending; stats: what the device call says about its launch
    (k_max, stage A's row parts, data batches, the most compactions of a workgroup, stage B's parts and rows per part, the scratch budget, the
    device's microseconds in the three stages: tail_us, body_us, fit_us) and,
    per datum, body_n, body_m, body_s: the rows outside the tail and the log-sum-exp body_m + log(body_s) of their -l"""
    __slots__ = ()

    def __str__(self):
        bad = [("NaN", self.n_nan), ("-inf", self.n_neg_inf), ("+inf", self.n_pos_inf)]
        rows = [("elpd_loo", "%.6g" % self.elpd_loo), ("se", "%.6g" % self.se), ("p_loo", "%.6g" % self.p_loo), ("lppd", "%.6g" % self.lppd),
                ("looic", "%.6g" % self.looic), ("n (draws)", "%d" % self.n), ("n_data", "%d" % len(self.lppd_i)),
                ("data with pareto_k > %.1f" % BAD_K, "%d" % self.n_bad_k)]
        worst = [int(i) for i in np.argsort(-np.nan_to_num(self.pareto_k, nan=-np.inf, posinf=np.inf)) if self.pareto_k[i] > BAD_K][:5]
        if worst:
            rows.append(("  the largest: datum (pareto_k)", ", ".join("%d (%.3g)" % (i, self.pareto_k[i]) for i in worst)))
        rows += [("data with a %s value" % name, "%d" % int(np.count_nonzero(c))) for name, c in bad]
        width = max(len(k) for k, _ in rows)
        return "\n".join("%-*s  %s" % (width, k, v) for k, v in rows)


def check_r_eff(who, r_eff, n_data):
    """-> (n_data,) float64: r_eff, a scalar or one value per datum, finite and > 0"""
    r = np.asarray(r_eff, dtype=np.float64)
    if r.ndim == 0:
        r = np.full(n_data, float(r))
    if r.shape != (n_data,):
        raise ValueError("%s: r_eff must be a scalar or have shape (%d,) (got %r)" % (who, n_data, r.shape))
    if not (np.isfinite(r).all() and (r > 0).all()):
        raise ValueError("%s: r_eff must be finite and > 0" % who)
    return np.ascontiguousarray(r)


def finish_loo(waic, rec, stats, tails):
    """waic: the PosteriorWaic of the window (lppd_i and the counters); rec (LOO_FIELDS, n_data): bpm_loo's records -> PosteriorLoo"""
    from . import _lib as L
    bad = (waic.n_nan + waic.n_neg_inf + waic.n_pos_inf) > 0
    elpd_i = np.where(bad, np.nan, rec[L.LOO_ELPD])
    k = np.where(bad, np.nan, rec[L.LOO_K])
    tail_len = np.where(bad, 0, np.ascontiguousarray(rec[L.LOO_TAIL_LEN]).view(np.int64))
    lppd_i = waic.lppd_i
    with np.errstate(invalid="ignore"):
        p_i = lppd_i - elpd_i
        elpd, p_loo, lppd = np.sum(elpd_i), np.sum(p_i), np.sum(lppd_i)
        se = np.sqrt(len(elpd_i) * np.var(elpd_i))
        n_bad = int(np.count_nonzero(k > BAD_K))
    st = dict(stats)
    st["body_n"] = np.ascontiguousarray(rec[L.LOO_BODY_N]).view(np.int64).copy()
    st["body_m"], st["body_s"], st["sigma"] = rec[L.LOO_BODY_M].copy(), rec[L.LOO_BODY_S].copy(), rec[L.LOO_SIGMA].copy()
    return PosteriorLoo(elpd_i, k, lppd_i, p_i, tail_len, waic.n_nan, waic.n_neg_inf, waic.n_pos_inf, float(elpd), float(p_loo), float(lppd),
                        float(se), float(-2.0 * elpd), n_bad, int(waic.n), tails, st)


def compute_loo(eng, allgather, pw, n_burn, n_chains, r_eff=1.0, tails=False):
    """The driver of param_est_loo on one rank: eng.pointwise gives lppd_i and the counters exactly as param_est_waic has them, eng.loo the
    rest.  -> PosteriorLoo"""
    if not isinstance(pw, HipPointwise):
        raise TypeError("%s: pw must be a HipPointwise (got %s)" % (WHO_LOO, type(pw).__name__))
    from .rank_diagnostics import check_single_rank
    check_single_rank(WHO_LOO, len(allgather(None)))
    n_burn = check_n_burn(WHO_LOO, n_burn)
    r = check_r_eff(WHO_LOO, r_eff, pw.n_data)
    if eng.window_rows(n_burn) == 0:
        raise empty_window(WHO_LOO, n_burn)
    rec, stats, tl = eng.loo(pw, n_burn, r, tails=bool(tails))       # (refuses a kept set beyond the budget before it compiles or allocates)
    waic = compute(eng.pointwise, allgather, pw, n_burn, n_chains, eng.history_rows())
    return finish_loo(waic, rec, stats, tl)


def compare_loo(a, b):
    """-> (elpd_diff, se_diff) of two PosteriorLoo over the same data and as many draws: elpd_diff = a.elpd_loo - b.elpd_loo (positive: a
    predicts better), se_diff = sqrt(n_data * np.var(a.elpd_loo_i - b.elpd_loo_i)) (Vehtari, Gelman and Gabry 2017, eq. 24).  Host
    arithmetic only."""
    for x in (a, b):
        if not isinstance(x, PosteriorLoo):
            raise TypeError("compare_loo: both arguments must be PosteriorLoo (got %s)" % type(x).__name__)
    if len(a.elpd_loo_i) != len(b.elpd_loo_i):
        raise ValueError("compare_loo: the results are over %d and %d data points; both must be over the same data" % (len(a.elpd_loo_i), len(b.elpd_loo_i)))
    if a.n != b.n or a.n <= 0:
        raise ValueError("compare_loo: the results are over %d and %d draws; both must be over the same number, more than 0" % (a.n, b.n))
    with np.errstate(invalid="ignore"):
        diff = a.elpd_loo_i - b.elpd_loo_i
        return float(a.elpd_loo - b.elpd_loo), float(np.sqrt(len(diff) * np.var(diff)))
