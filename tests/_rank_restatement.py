"""What tests/test_rank_diagnostics_host.py and tests/test_gpu_rank_diagnostics.py share: the NumPy / SciPy restatement of the rank-normalized
diagnostics (bipymc_amd/rank_diagnostics.py's definitions: scipy.stats.rankdata(method="average"), scipy.special.ndtri, np.median,
np.quantile) and the expected RankDiagnostics from tests/test_diagnostics_host.reference applied to each transformed array.  A plain module."""
import os
import sys

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_diagnostics_host import reference  # noqa: E402

PROB = (0.05, 0.95)
FIELDS = ("r_hat", "r_hat_bulk", "r_hat_tail", "ess_bulk", "ess_tail", "ess_lower", "ess_upper")


def split_rows(X, g0=0):
    """X (G, N, d) -> (2n, N, d): rows [g0, g0 + n) then [G - n, G), n = (G - g0) // 2 (an odd window drops its middle row)"""
    X = np.asarray(X, dtype=np.float64)
    G = X.shape[0]
    n = (G - g0) // 2
    return np.concatenate([X[g0:g0 + n], X[G - n:]], axis=0)


def pooled(W, f):
    """f over the S pooled values of every coordinate of W (rows, N, d) -> the same shape"""
    flat = W.reshape(-1, W.shape[-1])
    return np.stack([f(flat[:, k]) for k in range(flat.shape[1])], axis=1).reshape(W.shape)


def ranks(W):
    """average ranks, 1-based; a coordinate with a NaN is NaN throughout (rankdata's nan_policy="propagate")"""
    return pooled(W, lambda c: rankdata(c, method="average"))


def z_of(r):
    S = r.shape[0] * r.shape[1]
    return ndtri((r - 0.375) / (S + 0.25))


def restate(X, g0=0, prob=PROB):
    """-> dict: split (the split rows), rank, bulk, rank_folded, folded, lower, upper (all (2n, N, d)), median (d,), quantiles (2, d)"""
    W = split_rows(X, g0)
    flat = W.reshape(-1, W.shape[-1])
    with np.errstate(invalid="ignore"):
        med = np.median(flat, axis=0)
        q = np.quantile(flat, prob, axis=0)
        r = ranks(W)
        rf = ranks(np.abs(W - med))
        lower, upper = (W <= q[0]).astype(np.float64), (W <= q[1]).astype(np.float64)
    return dict(split=W, rank=r, bulk=z_of(r), rank_folded=rf, folded=z_of(rf), lower=lower, upper=upper, median=med, quantiles=q)


def expected(X, g0=0, prob=PROB, max_lag=None):
    """-> (restate(...), dict of test_diagnostics_host.reference per transformed array, dict of the RankDiagnostics fields)"""
    t = restate(X, g0, prob)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = {name: reference(t[name], max_lag=max_lag) for name in ("bulk", "folded", "lower", "upper")}
        f = dict(r_hat_bulk=ref["bulk"]["r_hat"], r_hat_tail=ref["folded"]["r_hat"], ess_bulk=ref["bulk"]["ess"], ess_lower=ref["lower"]["ess"],
                 ess_upper=ref["upper"]["ess"])
        f["r_hat"] = np.maximum(f["r_hat_bulk"], f["r_hat_tail"])
        f["ess_tail"] = np.minimum(f["ess_lower"], f["ess_upper"])
    f["ess_capped"] = ref["bulk"]["capped"] | ref["folded"]["capped"] | ref["lower"]["capped"] | ref["upper"]["capped"]
    return t, ref, f


def check_diagnostics(got, X, g0=0, prob=PROB, max_lag=None, r_hat_rtol=1e-10, ess_rtol=1e-8):
    """got: a RankDiagnostics of the history X.  The project's criteria (tests/test_gpu_diagnostics.py): r_hat within 1e-10 relative; ess
    within 1e-8 where the pair sum that ended Geyer's sequence is further than 1e-6 from zero (closer, rounding may end it either way), which
    must hold for at least 80 % of the coordinates that are not NaN; capped equal.  NaN where the restatement is NaN.  -> the restatement"""
    t, ref, f = expected(X, g0, prob, max_lag)
    d = X.shape[-1]
    N = X.shape[1]
    n = (X.shape[0] - g0) // 2
    assert (got.n_half_chains, got.n_draws, tuple(got.window)) == (2 * N, n, (g0, X.shape[0]))
    assert np.array_equal(got.median, t["median"], equal_nan=True), (got.median, t["median"])
    assert np.array_equal(got.quantiles, t["quantiles"], equal_nan=True), (got.quantiles, t["quantiles"])
    for name in FIELDS:
        g = getattr(got, name)
        assert g.shape == (d,) and np.array_equal(np.isnan(g), np.isnan(f[name])), (name, g, f[name])
    live = ~np.isnan(f["r_hat"])
    for name in ("r_hat", "r_hat_bulk", "r_hat_tail"):
        err = np.abs(getattr(got, name)[live] / f[name][live] - 1.0)
        print(name, "largest relative error", err.max() if err.size else 0.0)
        np.testing.assert_allclose(getattr(got, name)[live], f[name][live], rtol=r_hat_rtol, atol=0.0, err_msg=name)
    margin = {"ess_bulk": ref["bulk"]["margin"], "ess_lower": ref["lower"]["margin"], "ess_upper": ref["upper"]["margin"]}
    margin["ess_tail"] = np.minimum(margin["ess_lower"], margin["ess_upper"])
    for name in ("ess_bulk", "ess_lower", "ess_upper", "ess_tail"):
        ok = live & ~np.isnan(f[name]) & (margin[name] > 1e-6)
        assert ok.sum() >= 0.8 * (live & ~np.isnan(f[name])).sum(), (name, margin[name])
        err = np.abs(getattr(got, name)[ok] / f[name][ok] - 1.0)
        print(name, "largest relative error", err.max() if err.size else 0.0, "smallest margin", margin[name][ok].min() if ok.any() else None)
        np.testing.assert_allclose(getattr(got, name)[ok], f[name][ok], rtol=ess_rtol, atol=0.0, err_msg=name)
    assert np.array_equal(got.ess_capped[live], f["ess_capped"][live])
    return t
