"""Every per-coordinate statistic of the resident history with one non-finite value in it: the outputs that belong to the other coordinates are
the bits of the clean run on the same handle, the poisoned coordinate's own outputs are what NumPy gives on get_history() (each statistic's
existing comparison with NumPy, run on the poisoned history).

Shapes: N = 10, d = 3, G = 41 (ld = 4: a padding column; the classic kernels' only column group is ragged; an odd window) and N = 7, d = 5,
G = 40 (an odd number of chains).  One NaN (generation 5, the first half of the diagnostics' window) or one +inf (generation 27, the second
half) at (chain 0, coordinate 0), (chain 0, coordinate d - 1), (chain N - 1, coordinate 0) or (chain 1, coordinate 1).

What couples coordinates, legitimately: the log-likelihood of a row is a function of the whole row and set_history recomputes it, so the
poisoned row's ln-like is not finite -- ll_mean / ll_min / ll_max of its bin and chain_ll are compared with NumPy on get_loglike_history()
instead of with the clean run; best_ll / best_x / best_row are chosen among the ln-likes that are not NaN and stay those of the clean run
(the poisoned rows are not the best row).  posterior_summary's mean of a coordinate with an inf is NaN, as every split-chain moment of
such a coordinate is, where np.mean is +inf.  param_est_hist with range=None refuses a column that is not finite, as np.histogram does."""
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _rank_restatement as RR  # noqa: E402
import _summary_restatement as SR  # noqa: E402
import test_covariance_host as TC  # noqa: E402
import test_derived_host as TD  # noqa: E402
import test_histograms_host as TH  # noqa: E402
import test_traces_host as TT  # noqa: E402
from _history_cases import _engine, _over  # noqa: E402
from test_diagnostics_host import _ar1  # noqa: E402

SHAPES = [(10, 3, 41), (7, 5, 40)]
POISON = [(np.nan, 5), (np.inf, 27)]            # (value, generation)
Q = (0.05, 0.5, 0.95)
HDI_PROBS = (0.5, 0.94)
HIST = dict(bins=8, range=(-6.0, 6.0), pairs="all", bins2d=4)
EVERY = 7
FN_SRC = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    for (int k = 0; k < d; ++k) out[k] = p[0] * x[k] + p[1];
}"""


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) if a.dtype.kind == "f" else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _positions(N, d):
    return [(0, 0), (0, d - 1), (N - 1, 0), (1, 1)]


def _n_burn(N):
    return 2 * N + 3                             # a partial first generation


def _fn(d):
    from bipymc_amd import HipFunction
    return HipFunction(FN_SRC, n_out=d, params=[2.0, 1.0])


# ---- the statistics: name -> (s, e) -> (the result, {field: array with the coordinate on its LAST axis}) --------------------------------
def _fields(r, names):
    return r, dict((f, np.asarray(getattr(r, f))) for f in names)


def _diag(s, e):
    return _fields(s.convergence_diagnostics(), ("r_hat", "ess", "tau", "ess_capped", "lags_used"))


def _rank(s, e):
    return _fields(s.convergence_diagnostics_rank(), RR.FIELDS + ("median", "quantiles", "ess_capped"))


def _summary(s, e):
    return _fields(s.posterior_summary(), ("mean", "sd", "hdi_lo", "hdi_hi", "median", "quantiles", "mcse_mean", "mcse_sd", "ess_mean", "ess_sd",
                                           "ess_bulk", "ess_tail", "r_hat", "r_hat_classic", "ess_capped", "n_nan"))


def _hdi(s, e):
    return _fields(s.param_est_hdi(n_burn=_n_burn(e.n_chains), prob=HDI_PROBS), ("lo", "hi", "n_nan"))


def _quantiles(s, e):
    q = s.param_est_quantiles(n_burn=_n_burn(e.n_chains), q=Q)
    return q, dict(q=q)


def _hist(s, e):
    r = s.param_est_hist(n_burn=_n_burn(e.n_chains), **HIST)
    return r, dict(counts=r.counts.T, edges=r.edges.T)


def _trace(s, e):
    r = s.param_est_trace(n_burn=_n_burn(e.n_chains), every=EVERY, chains=[0, e.n_chains - 1])
    return _fields(r, ("mean", "sd", "min", "max", "n_nan", "chain_x", "best_x"))


def _derived(s, e):
    return _fields(s.param_est_fn(_fn(e.dim), n_burn=_n_burn(e.n_chains)), ("mean", "sd", "min", "max", "n_nan"))


def _cov(s, e):
    r = s.param_est_cov(n_burn=_n_burn(e.n_chains))
    return r, dict(mean=r.mean)


def _moments(s, e):
    count, s1, s2, shift = e.reduce_moments(_n_burn(e.n_chains))
    return (count, s1, s2, shift), dict(s1=s1, s2=s2, shift=shift)


STATS = dict(convergence_diagnostics=_diag, convergence_diagnostics_rank=_rank, posterior_summary=_summary, param_est_hdi=_hdi,
             param_est_quantiles=_quantiles, param_est_hist=_hist, param_est_trace=_trace, param_est_fn=_derived, param_est_cov=_cov,
             reduce_moments=_moments)


# ---- the poisoned coordinate's own outputs (and everything else once more) against NumPy on what the handle holds ------------------------
def _own(name, r, e, coord, clean):
    H, LL = e.get_history(), e.get_loglike_history()
    N, d = e.n_chains, e.dim
    nb = _n_burn(N)
    W = SR.param_est_window(H, nb)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if name == "convergence_diagnostics":
            assert np.isnan(r.r_hat[coord]) and np.isnan(r.ess[coord]) and np.isnan(r.tau[coord])
        elif name == "convergence_diagnostics_rank":
            RR.check_diagnostics(r, H)
        elif name == "posterior_summary" and np.isinf(H[:, :, coord]).any():
            # The split-chain moments of a coordinate with an inf are NaN, all of them (bipymc_amd/diagnostics.py), so the table's mean is
            # NaN where np.mean is +inf: the one column that is not NumPy's.  Every other column of that coordinate is.
            f = SR.expected(H)
            assert f["mean"][coord] == np.inf and np.isnan(r.mean[coord])
            for key in ("sd", "mcse_mean", "mcse_sd", "ess_mean", "ess_sd", "r_hat_classic"):
                assert np.isnan(f[key][coord]) and np.isnan(getattr(r, key)[coord]), key
            for key in ("hdi_lo", "hdi_hi", "median", "quantiles", "n_nan"):
                assert np.array_equal(getattr(r, key), f[key], equal_nan=True), key
            RR.check_diagnostics(r.rank, H)
        elif name == "posterior_summary":
            SR.check_summary(r, H)
        elif name == "param_est_hdi":
            lo, hi, n_nan = SR.hdi_columns(W, HDI_PROBS)
            assert np.array_equal(r.lo, lo, equal_nan=True) and np.array_equal(r.hi, hi, equal_nan=True) and np.array_equal(r.n_nan, n_nan)
        elif name == "param_est_quantiles":
            assert np.array_equal(r, np.quantile(W, Q, axis=0), equal_nan=True)
        elif name == "param_est_hist":
            TH.check_against_numpy(r, W, bins=HIST["bins"], rng=HIST["range"], bins2d=HIST["bins2d"])
        elif name == "param_est_trace":
            TT.check_against_numpy(r, H, LL, nb, EVERY, chains=[0, N - 1])
            for f in ("best_ll", "best_row"):
                assert getattr(r, f) == getattr(clean, f), f
        elif name == "param_est_fn":
            TD.check_summary(r, 2.0 * W + 1.0)
        elif name == "param_est_cov":
            # (test_covariance_host's rule: cov has NaN exactly where np.cov has -- the whole row and column; the mean is compared where
            # NumPy's is finite, and is not finite where NumPy's is not)
            TC.check_against_numpy(r, W)
            assert not np.isfinite(r.mean[coord]) and np.isnan(r.cov[coord]).all() and np.isnan(r.cov[:, coord]).all()
        elif name == "reduce_moments":
            count, s1, s2, shift = r
            assert count == len(W) and _same(shift, H[-1, 0])
            assert np.array_equal(s1[coord], np.sum(W[:, coord] - shift[coord]), equal_nan=True)
            assert np.array_equal(s2[coord], np.sum((W[:, coord] - shift[coord]) ** 2), equal_nan=True)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: "N%d-d%d-G%d" % p)
def case(request):
    N, d, G = request.param
    X = _ar1(G, N, np.linspace(0.0, 0.6, d), seed=40 + d)
    e = _engine(N, d)
    e.set_history(X, X[-1])
    s = _over(e)
    clean = dict((name, fn(s, e)) for name, fn in STATS.items())
    best = int(clean["param_est_trace"][0].best_row)
    for value, gen in POISON:
        for chain, coord in _positions(N, d):
            assert best != gen * N + chain                     # (the poisoned rows are not the best row)
    yield e, s, X, clean
    e.close()


@pytest.mark.parametrize("name", sorted(STATS))
def test_a_non_finite_value_moves_nothing_but_its_own_coordinate(case, name):
    e, s, X, clean = case
    N, d = e.n_chains, e.dim
    clean_r, clean_f = clean[name]
    try:
        for value, gen in POISON:
            for chain, coord in _positions(N, d):
                what = "%s: %r at generation %d, chain %d, coordinate %d" % (name, value, gen, chain, coord)
                Y = X.copy()
                Y[gen, chain, coord] = value
                e.set_history(Y, Y[-1])
                r, f = STATS[name](s, e)
                others = [k for k in range(d) if k != coord]
                for key in sorted(f):
                    assert _same(f[key][..., others], clean_f[key][..., others]), \
                        "%s changed %s of the other coordinates: %s -> %s" % (what, key, clean_f[key][..., others], f[key][..., others])
                if name == "param_est_cov":                    # entries outside the poisoned row and column
                    assert _same(r.cov[np.ix_(others, others)], clean_r.cov[np.ix_(others, others)]), what
                if name == "param_est_hist":                   # the pairs that exclude the column
                    keep = [p for p, (a, b) in enumerate(r.pairs) if coord not in (a, b)]
                    assert _same(r.counts2d[keep], clean_r.counts2d[keep]), what
                    with pytest.raises(ValueError, match="autodetected range of .* is not finite"):
                        s.param_est_hist(n_burn=_n_burn(N), bins=8)
                    # ... and without that column the autodetected ranges are NumPy's again
                    TH.check_against_numpy(s.param_est_hist(n_burn=_n_burn(N), bins=8, dims=others), SR.param_est_window(Y, _n_burn(N)), bins=8)
                _own(name, r, e, coord, clean_r)
    finally:
        e.set_history(X, X[-1])
