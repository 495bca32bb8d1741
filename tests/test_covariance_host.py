"""bipymc_amd/covariance.py without a GPU: covariance.compute driven by a NumPy stand-in for the two device calls (the same window and
shifted / centred sums, added as blocked partials in another order than NumPy's), on 1, 2 and 5 emulated ranks with uneven windows.

Tolerance (derived, not measured).  With y = x - c and u = 2^-53, any order of summing n products has |error(S2_ij)| <= gamma_n sum |y_i y_j|
<= gamma_n sqrt(sum y_i^2 sum y_j^2) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; gamma_n = n u / (1 - n u)), and
with c within rounding of the mean the right side is (n - 1) sqrt(C_ii C_jj) up to O(u).  The result under test and np.cov each carry such
an error, so element by element
    |cov - cov_numpy| <= 2 (n + 4) u sqrt(C_ii C_jj)              (C from NumPy)
    |mean - mean_numpy| <= 2 (n + 4) u (|mean| + sqrt(C_kk))
and against a np.longdouble two-pass covariance (n <= 10^5) the bound is (n + 4) u sqrt(C_ii C_jj).  No other tolerance appears here."""
import numpy as np
import pytest

from bipymc_amd import covariance as CV

U = 2.0 ** -53


def cov_bound(n, C, factor=2):
    sd = np.sqrt(np.diag(C))
    return factor * (n + 4) * U * np.outer(sd, sd)


def longdouble_cov(X):
    X = np.asarray(X, dtype=np.longdouble)
    m = X.mean(axis=0)
    Y = X - m
    return np.asarray((Y.T @ Y) / (X.shape[0] - 1), dtype=np.longdouble), m


def check_against_numpy(pc, X, long_double=True):
    n = X.shape[0]
    want = np.cov(X, rowvar=False).reshape(X.shape[1], X.shape[1])
    mean = np.mean(X, axis=0)
    assert pc.n == n
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(pc.cov), nan)
    err = np.abs(pc.cov - want)
    bound = cov_bound(n, np.where(nan, 0.0, want))
    assert np.all(err[~nan] <= bound[~nan]), float(np.max(err[~nan] / np.maximum(bound[~nan], 1e-300)))
    ok = ~np.isnan(mean) & np.isfinite(mean)
    assert np.all(np.abs(pc.mean - mean)[ok] <= (2 * (n + 4) * U * (np.abs(mean) + np.sqrt(np.diag(np.where(nan, 0.0, want)))))[ok])
    assert np.array_equal(pc.cov, pc.cov.T, equal_nan=True)
    if long_double and not nan.any():
        ref, _ = longdouble_cov(X)
        err = np.abs(pc.cov.astype(np.longdouble) - ref)
        assert np.all(err <= cov_bound(n, want, factor=1)), float(np.max(err / np.maximum(cov_bound(n, want, 1), 1e-300)))


class FakeRanks(object):
    """The device calls of R ranks over one super chain X (rows, dim) laid out as generations of N chains: rank r holds the chains
    [lo_r, hi_r) of every generation.  Sums are formed as 256 blocked partials added last to first."""

    def __init__(self, X, N, R):
        self.X = np.asarray(X, dtype=np.float64)
        self.N = N
        cuts = np.linspace(0, N, R + 1).astype(int)
        if R > 1:
            cuts[1] = max(1, cuts[1] - 1)       # uneven
        self.cuts = cuts
        self.R = R
        self.centers = []

    def _rows(self, r, n_burn):
        idx = np.arange(self.X.shape[0])
        chain = idx % self.N
        return self.X[(idx >= n_burn) & (chain >= self.cuts[r]) & (chain < self.cuts[r + 1])]

    @staticmethod
    def _blocked(Y):
        parts = [b.sum(axis=0) for b in np.array_split(Y, 256)] if len(Y) else [np.zeros(Y.shape[1:])]
        tot = np.zeros(Y.shape[1:])
        for p in reversed(parts):
            tot = tot + p
        return tot

    def reduce_moments(self, n_burn):
        shift = self.X[-self.N].copy()          # chain 0's current state, the same on every rank
        out = []
        for r in range(self.R):
            Y = self._rows(r, n_burn) - shift
            out.append((len(Y), self._blocked(Y), self._blocked(Y * Y), shift))
        return out

    def reduce_cov(self, n_burn, center):
        self.centers.append(np.array(center))
        out = []
        for r in range(self.R):
            Y = self._rows(r, n_burn) - center
            with np.errstate(invalid="ignore"):
                s2 = self._blocked(Y[:, :, None] * Y[:, None, :]) if len(Y) else np.zeros((Y.shape[1],) * 2)
            out.append((len(Y), self._blocked(Y), s2))
        return out


def run(X, N, R, n_burn=0):
    f = FakeRanks(X, N, R)
    return CV.compute(f.reduce_moments, f.reduce_cov, lambda x: x, n_burn, X.shape[1]), f


@pytest.mark.parametrize("R", [1, 2, 5])
@pytest.mark.parametrize("offset", [0.0, 50.0, 1e6])
def test_within_the_bound_of_numpy_and_long_double(R, offset):
    rs = np.random.RandomState(3)
    N, G, d = 50, 200, 6
    A = rs.normal(size=(d, d))
    X = rs.normal(size=(N * G, d)) @ A + offset
    for n_burn in (0, 7, N * 3 + 11):
        pc, _ = run(X, N, R, n_burn)
        check_against_numpy(pc, X[n_burn:])


def test_offset_posterior_needs_the_centre():
    """mean 10^6, sigma 1: the textbook one-pass formula sum x x^T / n - mean mean^T loses the covariance here; centring keeps the bound"""
    rs = np.random.RandomState(4)
    X = rs.normal(size=(100000, 4)) + 1e6
    pc, _ = run(X, 100, 2)
    check_against_numpy(pc, X)
    n = len(X)
    naive = (X.T @ X - n * np.outer(X.mean(axis=0), X.mean(axis=0))) / (n - 1)
    want = np.cov(X, rowvar=False)
    assert np.any(np.abs(naive - want) > cov_bound(n, want))


def test_every_rank_gets_the_same_bits_and_one_rank_agrees_within_the_bound():
    rs = np.random.RandomState(5)
    X = rs.normal(size=(64 * 40, 9)) * np.arange(1, 10) + 3.0
    res = {}
    for R in (1, 2, 5):
        f = FakeRanks(X, 64, R)
        # every emulated rank runs the driver on the same gathered parts
        per_rank = [CV.compute(f.reduce_moments, f.reduce_cov, lambda x: x, 64 * 2 + 5, 9) for _ in range(R)]
        for p in per_rank[1:]:
            assert np.array_equal(p.cov.view(np.uint64), per_rank[0].cov.view(np.uint64))
            assert np.array_equal(p.mean.view(np.uint64), per_rank[0].mean.view(np.uint64))
        res[R] = per_rank[0]
    want = np.cov(X[64 * 2 + 5:], rowvar=False)
    for R in (2, 5):
        assert np.all(np.abs(res[R].cov - res[1].cov) <= cov_bound(res[1].n, want))


def test_constant_and_tied_columns():
    rs = np.random.RandomState(6)
    X = rs.normal(size=(40 * 50, 5))
    X[:, 1] = 0.75                                     # (dyadic: NumPy's own mean of it is exact, so np.cov gives exactly 0 too)
    X[:, 3] = np.round(X[:, 3] * 2.0)
    pc, f = run(X, 40, 2)
    assert np.all(f.centers[-1][1] == 0.75)             # the centre of a constant column is the constant
    assert np.all(pc.cov[1, :] == 0.0) and np.all(pc.cov[:, 1] == 0.0)
    want = np.cov(X, rowvar=False)
    assert np.all(want[1, :] == 0.0)
    assert pc.mean[1] == 0.75
    check_against_numpy(pc, X)
    c = pc.corr()
    assert np.all(np.isnan(c[1, :])) and np.all(np.isnan(c[:, 1]))
    keep = [0, 2, 3, 4]
    assert np.all(np.diag(c)[keep] == 1.0)
    sd = np.sqrt(np.diag(pc.cov)[keep])
    assert np.array_equal(c[np.ix_(keep, keep)][~np.eye(4, dtype=bool)], (pc.cov[np.ix_(keep, keep)] / np.outer(sd, sd))[~np.eye(4, dtype=bool)])
    assert np.array_equal(c, c.T, equal_nan=True)


def test_nan_and_inf_columns():
    rs = np.random.RandomState(7)
    X = rs.normal(size=(30 * 20, 5))
    X[17, 1] = np.nan
    X[:40, 3] = np.inf
    X[40:60, 3] = -np.inf
    with np.errstate(invalid="ignore"):
        pc, _ = run(X, 30, 2)
        want = np.cov(X, rowvar=False)
    assert np.array_equal(np.isnan(pc.cov), np.isnan(want))
    assert np.isnan(want[1]).all() and np.isnan(want[3]).all() and not np.isnan(want[0, 0])
    with np.errstate(invalid="ignore"):
        check_against_numpy(pc, X, long_double=False)
    c = pc.corr()
    assert np.isnan(c[1]).all() and np.isnan(c[:, 3]).all() and c[0, 0] == 1.0


def test_errors():
    X = np.random.RandomState(8).normal(size=(10 * 4, 3))
    with pytest.raises(ValueError, match="window is empty"):
        run(X, 10, 2, 40)
    with pytest.raises(ValueError, match="window is empty"):
        run(X, 10, 1, 10 ** 9)
    with pytest.raises(ValueError, match="at least 2 rows"):
        run(X, 10, 2, 39)
    with pytest.raises(ValueError, match="n_burn must be >= 0"):
        run(X, 10, 1, -1)
    pc, _ = run(X, 10, 2, 38)
    check_against_numpy(pc, X[38:])


def test_exported_from_the_package():
    import bipymc_amd
    assert bipymc_amd.PosteriorCovariance is CV.PosteriorCovariance
    pc = bipymc_amd.PosteriorCovariance(np.zeros(2), np.array([[4.0, 1.0], [1.0, 1.0]]), 10)
    assert np.array_equal(pc.corr(), np.array([[1.0, 0.5], [0.5, 1.0]]))
