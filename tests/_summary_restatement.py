"""What tests/test_summary_host.py and tests/test_gpu_summary.py share: the NumPy restatement of bipymc_amd/summary.py's definitions (the
highest-density interval, mean, sd, the Monte Carlo standard errors) with the ESS through tests/test_diagnostics_host.reference, like
tests/_rank_restatement.py, and the tolerances of the GPU comparison with their derivation.  A plain module."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _rank_restatement as RR  # noqa: E402
from test_diagnostics_host import reference  # noqa: E402

EPS = 2.0 ** -52
R_HAT_RTOL, ESS_RTOL, ESS_MARGIN, ESS_SHARE = 1e-10, 1e-8, 1e-6, 0.8      # the project's criteria (tests/_rank_restatement.check_diagnostics)


def hdi_offset(p, S):
    return min(int(np.floor(p * S)), S - 1)


def hdi(values, p):
    """the definition, for one coordinate: values (S,) -> (lo, hi)"""
    v = np.asarray(values, dtype=np.float64) + 0.0                 # (-0.0 and +0.0 are one value)
    S = len(v)
    if np.isnan(v).any():
        return np.nan, np.nan
    s = np.sort(v)
    m = hdi_offset(p, S)
    with np.errstate(invalid="ignore"):
        w = s[m:] - s[:S - m]
    isnan = np.isnan(w)
    i = int(np.argmax(isnan)) if isnan.any() else int(np.argmin(w))      # the first NaN, else the first of the smallest
    return s[i], s[i + m]


def hdi_columns(flat, probs):
    """flat (S, d) -> (lo (len(probs), d), hi (len(probs), d), n_nan (d,))"""
    flat = np.asarray(flat, dtype=np.float64)
    out = np.array([[hdi(flat[:, k], p) for k in range(flat.shape[1])] for p in probs])
    return out[:, :, 0], out[:, :, 1], np.isnan(flat).sum(axis=0)


def param_est_window(X, n_burn):
    """X (G, N, d) -> param_est(n_burn)[2]: the super-chain rows >= n_burn, (rows, d)"""
    return np.asarray(X, dtype=np.float64).reshape(-1, X.shape[-1])[n_burn:]


def expected(X, g0=0, hdi_prob=0.94, prob=RR.PROB, max_lag=None):
    """-> dict of the PosteriorSummary fields of the history X (G, N, d) and what the tolerances need: ref_mean / ref_sd (the references of
    x and of d = (x - mean)^2), abs_mean (mean |x|), shift_ratio (max (d - mean(d))^2 / var(d))"""
    W = RR.split_rows(X, g0)
    flat = W.reshape(-1, W.shape[-1])
    S = len(flat)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = np.mean(flat, axis=0)
        sd = np.std(flat, axis=0, ddof=1)
        D = (W - mean) ** 2
        dflat = D.reshape(S, -1)
        mean_d, var_d = np.mean(dflat, axis=0), np.var(dflat, axis=0)
        ref_mean, ref_sd = reference(W, max_lag=max_lag), reference(D, max_lag=max_lag)
        rank = RR.expected(X, g0, prob, max_lag)
        lo, hi, n_nan = hdi_columns(flat, [hdi_prob])
        f = dict(mean=mean, sd=sd, hdi_lo=lo[0], hdi_hi=hi[0], median=rank[0]["median"], quantiles=rank[0]["quantiles"], n_nan=n_nan,
                 ess_mean=ref_mean["ess"], r_hat_classic=ref_mean["r_hat"], ess_sd=ref_sd["ess"], ess_bulk=rank[2]["ess_bulk"],
                 ess_tail=rank[2]["ess_tail"], r_hat=rank[2]["r_hat"], mcse_mean=sd / np.sqrt(ref_mean["ess"]),
                 mcse_sd=np.sqrt(((var_d / ref_sd["ess"]) / mean_d) / 4.0),
                 ess_capped=ref_mean["capped"] | ref_sd["capped"] | rank[2]["ess_capped"])
        f.update(ref_mean=ref_mean, ref_sd=ref_sd, rank=rank, abs_mean=np.mean(np.abs(flat), axis=0),
                 shift_ratio=np.max((dflat - mean_d) ** 2, axis=0) / var_d, S=S, n=W.shape[0] // 2, m=2 * W.shape[1], D=D, split=W)
    return f


# ---- the tolerances of the GPU comparison (derived in tests/test_summary_host.test_gpu_tolerances_follow_from_the_formats) ---------------
def sum_terms(n, m):
    """additions on the longest path of either side's sum of the S = m n values: the device's half-chain sums of n terms and their m-term
    combination, in any order; NumPy's pairwise sum is shorter"""
    return n + m + 8


def mean_atol(n, m, abs_mean):
    """|fl(sum x) - sum x| <= terms * eps * sum |x| for a sum of that many additions on its longest path in any order (Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2), on each side: 2 * terms * eps * mean |x|"""
    return 2.0 * sum_terms(n, m) * EPS * abs_mean


def sd_rtol(n, m):
    """The sum of squares about the mean is a sum of non-negative terms, so the same bound is relative: terms * eps on each side, plus a few
    roundings for the squares and the second-order effect of the mean's error; the square root halves it: (2 * terms + 16) / 2 * eps"""
    return (sum_terms(n, m) + 8) * EPS


def mcse_mean_rtol(n, m):
    """sd / sqrt(ess_mean): the sd's bound plus half the ESS tolerance"""
    return sd_rtol(n, m) + 0.5 * ESS_RTOL


def mcse_sd_rtol(S, shift_ratio):
    """sqrt(var(d) / ess_sd / mean(d) / 4): half of (var(d)'s + the ESS's + mean(d)'s).  mean(d) is a sum of S non-negative terms: S * eps
    on each side at worst.  var(d) on the device is s2 / S - (s1 / S)^2 about a shift that is one of the values of d: s2 / S = var(d) +
    (shift - mean(d))^2, so the sum's relative error S * eps is amplified by at most 1 + 2 * max (d - mean(d))^2 / var(d) = 1 + 2 *
    shift_ratio (the subtrahend carries as much again); the reference's own d differs by the mean's rounding, which is second order."""
    var_rtol = 2.0 * (S + 8) * EPS * (1.0 + 2.0 * shift_ratio)
    return 0.5 * (var_rtol + ESS_RTOL + 2.0 * (S + 8) * EPS)


def check_ess(name, got, ref):
    """the project's rule for one ESS column against one test_diagnostics_host.reference: NaN where the reference is NaN; within ESS_RTOL where
    the pair sum that ended Geyer's sequence is further than ESS_MARGIN from zero, which must hold for ESS_SHARE of the live coordinates"""
    want = ref["ess"]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (name, got, want)
    live = ~np.isnan(want)
    ok = live & (ref["margin"] > ESS_MARGIN)
    assert ok.sum() >= ESS_SHARE * live.sum(), (name, ref["margin"])
    err = np.abs(got[ok] / want[ok] - 1.0)
    print(name, "largest relative error", err.max() if err.size else 0.0, "smallest margin", ref["margin"][ok].min() if ok.any() else None)
    np.testing.assert_allclose(got[ok], want[ok], rtol=ESS_RTOL, atol=0.0, err_msg=name)
    return ok


def check_summary(got, X, g0=0, hdi_prob=0.94, prob=RR.PROB, max_lag=None):
    """got: a PosteriorSummary of the history X.  hdi, median, quantiles, n_nan exact; r_hat / ESS by the project's criteria; mean, sd and
    the two standard errors at the tolerances above.  -> expected(...)"""
    f = expected(X, g0, hdi_prob, prob, max_lag)
    n, m, S = f["n"], f["m"], f["S"]
    assert (got.n_half_chains, got.n_draws, tuple(got.window)) == (m, n, (g0, X.shape[0]))
    for name in ("hdi_lo", "hdi_hi", "median", "quantiles", "n_nan"):
        assert np.array_equal(getattr(got, name), f[name], equal_nan=True), (name, getattr(got, name), f[name])
    RR.check_diagnostics(got.rank, X, g0, prob, max_lag)
    for name in ("ess_bulk", "ess_tail", "r_hat", "median", "quantiles"):
        assert getattr(got, name) is getattr(got.rank, name), name
    for name in ("mean", "sd", "mcse_mean", "mcse_sd", "r_hat_classic"):
        assert np.array_equal(np.isnan(getattr(got, name)), np.isnan(f[name])), (name, getattr(got, name), f[name])
    live = ~np.isnan(f["r_hat_classic"]) & ~np.isnan(f["r_hat"])
    np.testing.assert_allclose(got.r_hat_classic[live], f["r_hat_classic"][live], rtol=R_HAT_RTOL, atol=0.0)
    ok_mean = check_ess("ess_mean", got.ess_mean, f["ref_mean"])
    ok_sd = check_ess("ess_sd", got.ess_sd, f["ref_sd"])
    fin = np.isfinite(f["mean"])
    print("mean: largest error / bound", np.max(np.abs(got.mean[fin] - f["mean"][fin]) / mean_atol(n, m, f["abs_mean"][fin])))
    assert np.all(np.abs(got.mean[fin] - f["mean"][fin]) <= mean_atol(n, m, f["abs_mean"][fin]))
    fin = np.isfinite(f["sd"])
    print("sd: largest relative error", np.max(np.abs(got.sd[fin] / f["sd"][fin] - 1.0)), "bound", sd_rtol(n, m))
    np.testing.assert_allclose(got.sd[fin], f["sd"][fin], rtol=sd_rtol(n, m), atol=0.0)
    print("mcse_mean: largest relative error", np.max(np.abs(got.mcse_mean[ok_mean] / f["mcse_mean"][ok_mean] - 1.0)), "bound", mcse_mean_rtol(n, m))
    np.testing.assert_allclose(got.mcse_mean[ok_mean], f["mcse_mean"][ok_mean], rtol=mcse_mean_rtol(n, m), atol=0.0)
    for k in np.nonzero(ok_sd)[0]:
        bound = mcse_sd_rtol(S, f["shift_ratio"][k])
        print("mcse_sd[%d]: relative error" % k, abs(got.mcse_sd[k] / f["mcse_sd"][k] - 1.0), "bound", bound)
        np.testing.assert_allclose(got.mcse_sd[k], f["mcse_sd"][k], rtol=bound, atol=0.0)
    assert np.array_equal(got.ess_capped[live], f["ess_capped"][live])
    return f

