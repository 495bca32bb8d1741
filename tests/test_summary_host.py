"""The posterior summary on the host (bipymc_amd/summary.py + HistoryStatistics.param_est_hdi / posterior_summary): the NumPy restatement of
tests/_summary_restatement.py against hand-worked cases and known distributions, the finishing layer over NumPy stand-ins for the device
calls, the argument errors, the multi-rank refusal and the derivation of the tolerances tests/test_gpu_summary.py compares at."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _rank_restatement as RR  # noqa: E402
import _summary_restatement as SR  # noqa: E402
from bipymc_amd import rank_diagnostics as RK  # noqa: E402
from bipymc_amd import summary as SM  # noqa: E402
from test_diagnostics_host import BlockParts, _ar1  # noqa: E402
from test_rank_diagnostics_host import Comm, FakeRanked, FakeRankEngine, Sampler  # noqa: E402

INF = np.inf


# ---- the restatement against hand-worked cases -------------------------------------------------------------------------------------------
def test_ties_in_the_width_take_the_first_index():
    # sorted 0 1 2 3 10 11 12 13, S = 8, p = 0.5: m = 4, widths 10 10 10 10 -> i* = 0; p = 0.3: m = 2, widths 2 2 8 9 2 2 -> i* = 0
    v = np.array([12.0, 0.0, 3.0, 10.0, 1.0, 13.0, 2.0, 11.0])
    assert SR.hdi(v, 0.5) == (0.0, 10.0)
    assert SR.hdi(v, 0.3) == (0.0, 2.0)
    # the smallest width is not the first one: sorted 0 5 6 7 20, m = floor(0.5 * 5) = 2, widths 6 2 14 -> i* = 1
    assert SR.hdi([20.0, 0.0, 6.0, 5.0, 7.0], 0.5) == (5.0, 7.0)
    # the rule is np.argmin's on the widths
    s = np.sort(v)
    assert int(np.argmin(s[4:] - s[:4])) == 0


def test_m_zero_is_the_smallest_value_and_minus_zero_is_plus_zero():
    # p * S < 1: m = 0, every width is 0 -> the first index: (min, min)
    assert SR.hdi_offset(1e-5, 25600) == 0 and SR.hdi_offset(0.1, 8) == 0
    assert SR.hdi([3.0, 1.0, 2.0], 0.2) == (1.0, 1.0)
    lo, hi = SR.hdi([0.0, -0.0, 5.0], 0.2)
    assert (lo, hi) == (0.0, 0.0) and not np.signbit(lo) and not np.signbit(hi)


def test_infinite_values_give_a_nan_width_at_its_first_index():
    # m = 0 with a -inf: w[0] = -inf - -inf = NaN -> i* = 0, the interval is (-inf, -inf)
    assert SR.hdi([1.0, -INF, 2.0, INF], 0.1) == (-INF, -INF)
    # sorted -inf -inf 0 1, m = 1: widths NaN inf 1 -> the NaN, not the smallest
    assert SR.hdi([0.0, -INF, 1.0, -INF], 0.3) == (-INF, -INF)
    # sorted 0 1 inf inf, m = 1: widths 1 inf NaN -> index 2
    assert SR.hdi([INF, 0.0, INF, 1.0], 0.3) == (INF, INF)
    # an inf width is an ordinary width: sorted -inf 0 1 5, m = 2: widths inf 5 -> (0, 5)
    assert SR.hdi([5.0, -INF, 1.0, 0.0], 0.5) == (0.0, 5.0)
    # NaN widths follow np.argmin's rule as well
    with np.errstate(invalid="ignore"):
        assert int(np.argmin(np.array([1.0, INF, INF - INF]))) == 2


def test_a_nan_gives_nan_and_is_counted():
    lo, hi = SR.hdi([1.0, np.nan, 2.0], 0.5)
    assert np.isnan(lo) and np.isnan(hi)
    flat = np.array([[1.0, np.nan], [2.0, 3.0], [0.0, np.nan]])
    lo, hi, n_nan = SR.hdi_columns(flat, [0.5, 0.9])
    assert lo.shape == hi.shape == (2, 2) and np.isnan(lo[:, 1]).all() and np.isnan(hi[:, 1]).all() and list(n_nan) == [0, 2]
    assert (lo[0, 0], hi[0, 0]) == (0.0, 1.0) and (lo[1, 0], hi[1, 0]) == (0.0, 2.0)


def test_the_offset_is_clamped_and_computed_in_doubles():
    # floor(p S) reaches S only at p = 1, which the callers refuse (for p <= 1 - 2^-53 and S < 2^53 the product rounds to S - 1 at most): the
    # clamp is what keeps i + m < S whatever is passed
    p = float(np.nextafter(1.0, 0.0))
    assert p < 1.0 and SR.hdi_offset(p, 2 ** 31 - 1) == 2 ** 31 - 2 and SR.hdi_offset(1.0, 4) == 3 and SM.hdi_offset(1.0, 4) == 3
    assert SR.hdi_offset(0.94, 25600) == 24064 and SR.hdi_offset(0.5, 25600) == 12800 and SR.hdi_offset(0.999, 4) == 3
    for p_, S in ((0.94, 25600), (0.3, 7), (0.7, 279), (1e-5, 32), (p, 2 ** 31 - 1)):
        assert SM.hdi_offset(p_, S) == SR.hdi_offset(p_, S)
    assert SR.hdi([4.0, 1.0, 2.0, 3.0], 0.999) == (1.0, 4.0)           # m = S - 1: the whole range


# ---- against known distributions -----------------------------------------------------------------------------------------------------------
def test_mcse_sd_of_independent_normals_is_sd_over_sqrt_2s():
    """Independent N(0, sigma^2) draws: d = (x - mean)^2 is sigma^2 chi^2_1, var(d) = 2 sigma^4, mean(d) = sigma^2, ess_sd = S, so mcse_sd =
    sqrt(2 sigma^4 / S / sigma^2 / 4) = sigma / sqrt(2 S).  The margin is the estimators' own sampling error.  Relative standard errors over S
    draws: of var^(d), sqrt((kurtosis(d) - 1) / S) with kurtosis(chi^2_1) = 15: sqrt(14 / S); of mean^(d), sqrt(var(d)) / mean(d) / sqrt(S) =
    sqrt(2 / S); of tau^ = S / ess^, sqrt(4 M / S) for a truncated sum of M autocorrelation lags each of variance 1 / S (Priestley 1981,
    6.2.1; Geyer's rule ends a white sequence within the first few pairs: M <= 8).  mcse_sd is the square root of their product and
    quotient: half the root of the sum of squares; the comparison sd / sqrt(2 S) adds sd's own sqrt(1 / (2 S)).  Four standard errors."""
    G, N = 401, 64
    X = np.random.RandomState(12).normal(size=(G, N, 3)) * np.array([1.0, 0.1, 30.0])
    f = SR.expected(X)
    S = f["S"]
    assert S == 25600
    rel_se = 0.5 * np.sqrt(14.0 / S + 2.0 / S + 4.0 * 8 / S) + np.sqrt(0.5 / S)
    err = np.abs(f["mcse_sd"] / (f["sd"] / np.sqrt(2.0 * S)) - 1.0)
    print("mcse_sd against sd / sqrt(2 S): relative differences", err, "four standard errors", 4 * rel_se)
    assert (err < 4 * rel_se).all()


def test_mcse_mean_of_an_ar1_chain_is_sd_times_the_known_factor():
    """A stationary AR(1) chain with coefficient phi has tau = (1 + phi) / (1 - phi), so mcse_mean = sd sqrt(tau / S).  Sampling error of the
    estimate: tau^ is a truncated sum of M autocorrelation lags, relative standard error sqrt(4 M / S) (as above), where Geyer's rule ends the
    sum once phi^t has sunk into the lags' noise 1 / sqrt(S): t = ln(sqrt(S)) / ln(1 / phi), 7.3 lags at phi = 0.5 and 48 at phi = 0.9 for S =
    25600, and the sum runs on for a few pairs: M = 2 t.  mcse_mean takes the root: half of it.  sd's own error sqrt(tau / (2 S)) is added.
    Four standard errors."""
    phis = np.array([0.0, 0.5, 0.9])
    X = _ar1(401, 64, phis, seed=11)
    f = SR.expected(X)
    S = f["S"]
    tau = (1.0 + phis) / (1.0 - phis)
    with np.errstate(divide="ignore"):
        M = np.maximum(8.0, 2.0 * np.log(np.sqrt(S)) / np.log(1.0 / phis))
    rel_se = 0.5 * np.sqrt(4.0 * M / S) + np.sqrt(tau / (2.0 * S))
    err = np.abs(f["mcse_mean"] / (f["sd"] * np.sqrt(tau / S)) - 1.0)
    print("mcse_mean against sd sqrt(tau / S): relative differences", err, "four standard errors", 4 * rel_se)
    assert (err < 4 * rel_se).all()


# ---- the finishing layer over NumPy stand-ins for the device calls -----------------------------------------------------------------------
class FakeScratch(FakeRanked):
    def reduce_moments(self, n_burn=0):
        flat = self.H.reshape(-1, self.H.shape[2])[n_burn:]
        shift = self.H[-1, 0].copy()                                  # (the state's first chain: the last row)
        with np.errstate(invalid="ignore"):
            return len(flat), (flat - shift).sum(axis=0), ((flat - shift) ** 2).sum(axis=0), shift


class FakeSummaryEngine(FakeRankEngine):
    """FakeRankEngine with the squared-deviation fill, the raw diagnostics and hdi as HipEngine states them"""

    def rank_history(self, g_lo, g_hi, kind, arg=None, positions=(), dst=None):
        own = dst is None
        if own:
            dst = FakeScratch(self.calls)
            self.made.append(dst)
        if kind != RK.KIND_SQDEV:
            try:
                return FakeRankEngine.rank_history(self, g_lo, g_hi, kind, arg, positions, dst)
            except BaseException:
                if own:
                    dst.close()                                       # (as HipEngine.rank_history: a handle it made itself)
                raise
        self.calls.append((g_lo, g_hi, kind, np.array(arg), tuple(positions), dst))
        if self.fail_at == len(self.calls):
            raise RuntimeError("bpm_rank_history: failed on purpose")
        with np.errstate(invalid="ignore"):
            dst.H = (RR.split_rows(self.X[:g_hi], g_lo) - np.asarray(arg)) ** 2
        dst.fail_diag = False
        return dst, np.empty((0, self.dim))

    def diag_split_moments(self, a, b):
        self._dg = BlockParts(self.X)
        return self._dg.split(a, b)

    def diag_autocov(self, t0, nl):
        return self._dg.autocov(t0, nl)

    def hdi(self, window, a, b, prob, positions=()):
        flat = RR.split_rows(self.X[:b], a).reshape(-1, self.dim) if window == 0 else SR.param_est_window(self.X, a)
        self.hdi_calls = getattr(self, "hdi_calls", []) + [(window, a, b, tuple(prob))]
        lo, hi, n_nan = SR.hdi_columns(flat, prob)
        return lo, hi, n_nan, len(flat), np.empty((0, self.dim))


def _history(G=81, N=8, seed=3):
    X = _ar1(G, N, [0.0, 0.5, 0.9, 0.3, -0.2], seed=seed)
    X[:, :4, 3] *= 3.0
    return X


def test_every_column_equals_its_definition():
    X = _history()
    e = FakeSummaryEngine(X)
    got = Sampler(e).posterior_summary(n_burn=8 * 2 + 3, hdi_prob=0.8, prob=(0.1, 0.9), max_lag=30)
    f = SR.check_summary(got, X, g0=3, hdi_prob=0.8, prob=(0.1, 0.9), max_lag=30)
    assert got.hdi_prob == 0.8 and got.prob == (0.1, 0.9) and got.window == (3, 81) and got.n_draws == 39 and got.n_half_chains == 16
    np.testing.assert_allclose(got.mcse_mean, f["mcse_mean"], rtol=1e-12)
    np.testing.assert_allclose(got.mcse_sd, f["mcse_sd"], rtol=1e-11)
    # ONE scratch handle took five fills -- z, folded z, two indicators, the squared deviations about the mean -- and was closed once
    assert [c[2] for c in e.calls] == [1, 2, 3, 3, 5] and len(e.made) == 1 and e.made[0].closed == 1
    assert all(c[5] is e.made[0] for c in e.calls[1:]) and np.array_equal(e.calls[4][3], got.mean)
    assert e.hdi_calls == [(0, 3, 81, (0.8,))]
    text = str(got)
    assert len(text.splitlines()) == 1 + 5 + 1 and "hdi_10%" in text and "hdi_90%" in text and "mcse_sd" in text and "r_hat" in text


def test_param_est_hdi_is_the_definition_over_param_ests_rows():
    X = _history()
    X[5, 2, 1] = np.nan
    s = Sampler(FakeSummaryEngine(X))
    got = s.param_est_hdi(n_burn=8 * 10 + 3, prob=(0.94, 0.5))
    lo, hi, n_nan = SR.hdi_columns(SR.param_est_window(X, 83), (0.94, 0.5))
    assert got.lo.shape == (2, 5) and np.array_equal(got.lo, lo, equal_nan=True) and np.array_equal(got.hi, hi, equal_nan=True)
    assert got.n == 81 * 8 - 83 and got.prob == (0.94, 0.5) and np.array_equal(got.n_nan, n_nan)
    one = s.param_est_hdi(prob=0.5)
    assert one.lo.shape == (5,) and np.isnan(one.lo[1]) and one.n_nan[1] == 1 and one.n == 81 * 8
    assert np.array_equal(one.lo[[0, 2]], SR.hdi_columns(X.reshape(-1, 5), [0.5])[0][0][[0, 2]])


@pytest.mark.parametrize("fail_at", [1, 3, 5])
def test_the_scratch_handle_is_closed_when_a_fill_raises(fail_at):
    e = FakeSummaryEngine(_history(), fail_at=fail_at)
    with pytest.raises(RuntimeError, match="failed on purpose"):
        Sampler(e).posterior_summary()
    assert len(e.made) == 1 and e.made[0].closed == 1
    # ... and convergence_diagnostics_rank itself still closes its handle when nobody asks for it
    e = FakeSummaryEngine(_history())
    Sampler(e).convergence_diagnostics_rank()
    assert [c[2] for c in e.calls] == [1, 2, 3, 3] and e.made[0].closed == 1


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,text", [(0.0, r"inside \(0, 1\) \(got 0.0\)"), (1.0, r"inside \(0, 1\) \(got 1.0\)"), (-0.1, "inside"), (np.nan, "inside"),
                                       ((0.5, 1.5), "inside"), ((), "0 probabilities given; one call takes 1 ... 8"),
                                       ((0.1,) * 9, "9 probabilities given; one call takes 1 ... 8"), ("wide", "prob must be a probability")])
def test_probabilities_are_validated_before_the_engine_is_touched(prob, text):
    s = Sampler(None)
    with pytest.raises(ValueError, match="param_est_hdi: .*" + text):
        s.param_est_hdi(prob=prob)
    with pytest.raises(ValueError, match="posterior_summary: .*" + text):
        s.posterior_summary(hdi_prob=prob)
    assert s.asked == []


def test_other_argument_errors():
    s = Sampler(None)
    with pytest.raises(ValueError, match="posterior_summary: prob must satisfy 0 < lo < hi < 1"):
        s.posterior_summary(prob=(0.9, 0.1))
    assert s.asked == []
    with pytest.raises(RuntimeError, match="posterior_summary: run_mcmc first"):
        s.posterior_summary()
    with pytest.raises(RuntimeError, match="param_est_hdi: run_mcmc first"):
        s.param_est_hdi()
    s = Sampler(FakeSummaryEngine(_history()))
    with pytest.raises(ValueError, match="posterior_summary: hdi_prob must be one probability"):
        s.posterior_summary(hdi_prob=(0.5, 0.9))
    with pytest.raises(ValueError, match="param_est_hdi: n_burn must be >= 0"):
        s.param_est_hdi(n_burn=-1)
    with pytest.raises(ValueError, match="posterior_summary: n_burn must be >= 0"):
        s.posterior_summary(n_burn=-1)
    with pytest.raises(ValueError, match=r"param_est_hdi: the window is empty \(n_burn = 648"):
        s.param_est_hdi(n_burn=81 * 8)
    with pytest.raises(RuntimeError, match="at least 4"):
        s.posterior_summary(n_burn=8 * 75)
    with pytest.raises(ValueError, match="max_lag must be >= 1"):
        s.posterior_summary(max_lag=0)
    assert all(h.closed == 1 for h in s._engine.made)


def test_two_ranks_are_refused_before_any_engine_call():
    s = Sampler(FakeSummaryEngine(_history()), comm=Comm(2))
    with pytest.raises(NotImplementedError, match="posterior_summary: pooled ranks are built on a single rank only .* 2 ranks"):
        s.posterior_summary()
    with pytest.raises(NotImplementedError, match="param_est_hdi: pooled ranks are built on a single rank only .* 2 ranks"):
        s.param_est_hdi()
    assert s.asked == [] and s._engine.calls == []


def test_every_sampler_class_has_the_methods_and_the_abi_the_entry_point():
    from bipymc_amd import DeMcMpi, DerivedHistory, DreamMpi, PosteriorHDI, PosteriorSummary, _lib
    from bipymc_amd.samplers import DeMc
    for cls in (DeMcMpi, DreamMpi, DeMc, DerivedHistory):
        assert callable(cls.param_est_hdi) and callable(cls.posterior_summary)
    assert PosteriorHDI is SM.PosteriorHDI and PosteriorSummary is SM.PosteriorSummary
    assert "bpm_hdi" in _lib.SIGNATURES and len(_lib.SIGNATURES["bpm_hdi"][1]) == 13
    assert RK.KIND_SQDEV == 5 and SM.MAX_PROB == 8
    text = open(os.path.join(HERE, "..", "bipymc_amd", "csrc", "ranks.h")).read()
    assert "RK_SQDEV = 5" in text and "constexpr int RK_MAX_PROB = 8;" in text


# ---- the tolerances tests/test_gpu_summary.py compares at ---------------------------------------------------------------------------------
def test_gpu_tolerances_follow_from_the_formats():
    """tests/_summary_restatement.py: mean_atol, sd_rtol, mcse_mean_rtol, mcse_sd_rtol, each with its reasoning.  Here they are evaluated at
    the GPU test's shape and checked where they can be without a device: sums taken in the device's order (half-chain by half-chain,
    sequentially, in float64) against the same sums in extended precision must lie inside them, and so must the shifted variance about the
    WORST shift the device could meet (the largest value of d)."""
    n, m, S = 200, 128, 25600
    assert SR.sum_terms(n, m) == 336
    assert SR.sd_rtol(n, m) == 344 * 2.0 ** -52 and SR.sd_rtol(n, m) < 1e-13
    assert SR.mcse_mean_rtol(n, m) == SR.sd_rtol(n, m) + 5e-9
    # independent normals: max (d - mean d)^2 / var d is about (2 ln S)^2 / 2 = 200 at S = 25600 -> 1e-8 at most, the order of the ESS tolerance
    assert SR.mcse_sd_rtol(S, 200.0) < 1e-8 and SR.mcse_sd_rtol(S, 0.0) > 0.5 * SR.ESS_RTOL
    X = _ar1(2 * n + 1, m // 2, [0.0, 0.9, 0.5], seed=7, offset=np.array([0.0, 1e3, -5.0]))
    W = RR.split_rows(X)
    halves = np.concatenate([W[:n], W[n:]], axis=1)                  # (n, m, d)
    flat = W.reshape(-1, 3)
    exact_mean = np.mean(flat.astype(np.longdouble), axis=0)
    exact_sd = np.sqrt(np.sum((flat.astype(np.longdouble) - exact_mean) ** 2, axis=0) / (S - 1))
    xbar = np.zeros((m, 3))
    for t in range(n):                                               # sequential sums, the longest path a device reduction could take
        xbar += halves[t]
    xbar /= n
    mean = np.zeros(3)
    for j in range(m):
        mean += xbar[j]
    mean /= m
    s2 = np.zeros((m, 3))
    for t in range(n):
        s2 += (halves[t] - xbar) ** 2
    s2 /= n - 1.0
    sd = SM.sd_of_split_moments(m, n, ((xbar - mean) ** 2).sum(axis=0), s2.sum(axis=0))
    abs_mean = np.mean(np.abs(flat), axis=0)
    assert np.all(np.abs(mean - exact_mean) <= 0.5 * SR.mean_atol(n, m, abs_mean))           # (half: the bound covers both sides)
    assert np.all(np.abs(np.mean(flat, axis=0) - exact_mean) <= 0.5 * SR.mean_atol(n, m, abs_mean))
    assert np.all(np.abs((sd / exact_sd).astype(np.float64) - 1.0) <= 0.5 * SR.sd_rtol(n, m))
    assert np.all(np.abs((np.std(flat, axis=0, ddof=1) / exact_sd).astype(np.float64) - 1.0) <= 0.5 * SR.sd_rtol(n, m))
    # the shifted variance of d about the worst shift, summed sequentially
    d = (flat - mean) ** 2
    exact_var = np.var(d.astype(np.longdouble), axis=0)
    shift = d.max(axis=0)
    s1, s2_ = np.zeros(3), np.zeros(3)
    for row in d:
        s1 += row - shift
        s2_ += (row - shift) ** 2
    got_mean, got_var = SM.shifted_mean_var(S, s1, s2_, shift)
    ratio = np.max((d - d.mean(axis=0)) ** 2, axis=0) / np.var(d, axis=0)
    bound = 2.0 * (S + 8) * SR.EPS * (1.0 + 2.0 * ratio)            # (mcse_sd_rtol's var_rtol)
    print("shifted variance about the worst shift: relative error", np.abs((got_var / exact_var).astype(np.float64) - 1.0), "bound", bound)
    assert np.all(np.abs((got_var / exact_var).astype(np.float64) - 1.0) <= bound)
    assert np.all(np.abs((got_mean / np.mean(d.astype(np.longdouble), axis=0)).astype(np.float64) - 1.0) <= 2.0 * (S + 8) * SR.EPS)
