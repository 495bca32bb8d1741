"""A derived history is a history (HistoryStatistics.derived_history / bpm_derive_history + the fill kernel of bipymc_amd/csrc/derive_rows.h).

The contract under test: with V = sampler.param_est_fn(fn, 0, values=True).values reshaped to (G, N, n_out), every method of the derived
history returns what the same method returns on a sampler whose history is V and whose log-likelihood history is the parent's.  So every
check hands V to the checker the statistic already has:
  values, log-likelihoods     bit for bit (NaN against NaN: test_gpu_derived._bits_equal)
  quantiles                   np.quantile on V, np.array_equal(..., equal_nan=True)
  histograms                  test_histograms_host.check_against_numpy: exact counts, edges bit for bit
  covariance                  test_covariance_host.check_against_numpy: within cov_bound
  traces                      test_traces_host.check_against_numpy: min / max / counts / best_* exact, mean and sd within trace_bound
  R-hat / ESS                 test_diagnostics_host.reference at tests/test_gpu_diagnostics.py's 1e-10 / 1e-8 relative, on the outputs whose
                              values are all finite and not constant (the reference itself returns NaN elsewhere); for R-hat of an output
                              far from the origin plus the rounding of the half-chain means, derived in _check_diagnostics
  param_est_fn on the derived history: test_gpu_derived._check (values bit for bit, summaries within trace_bound)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_covariance_host as TC  # noqa: E402
import test_histograms_host as TH  # noqa: E402
import test_traces_host as TT  # noqa: E402
from _history_cases import _dream_class, _engine, _over  # noqa: E402
from test_diagnostics_host import reference  # noqa: E402
from test_gpu_derived import (EXP_SRC, FIVE_SRC, WIDE_SRC, _bits_equal, _check, _five, _history_with_zero_denominators,  # noqa: E402
                              _layout)

Q = (0.05, 0.5, 0.95)
PAIR_SRC = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[1] + x[3];
    out[1] = x[0] * p[0] + ll;
}"""


def _pair():
    from bipymc_amd import HipFunction

    def py(X, ll, p):
        with np.errstate(all="ignore"):
            return np.stack([X[:, 1] + X[:, 3], X[:, 0] * p[0] + ll], axis=1)

    return HipFunction(PAIR_SRC, n_out=2, params=[0.5], python_fn=py)


def _values(s, fn):
    """V (G, N, n_out): the parent's own values of fn over its whole history"""
    v = s.param_est_fn(fn, 0, values=True).values
    return v.reshape(-1, s.n_chains, fn.n_out)


def _check_values(dh, V, LL):
    G, N, M = V.shape
    assert (dh.n_out, dh.dim, dh.n_chains, dh.history_rows) == (M, M, N, G)
    assert dh._engine.dim == M and dh._engine.n_chains == N and dh._engine.history_rows() == G
    _bits_equal(dh.param_est(0)[2], V.reshape(-1, M), "values")
    _bits_equal(dh._engine.get_history(), V, "history")
    _bits_equal(dh._engine.get_loglike_history(), LL, "ln-likes")
    _bits_equal(dh._engine.get_state(), V[-1], "state")               # (what bpm_set_history leaves: the last row)
    _bits_equal(dh._engine.get_loglike(), LL[-1], "ln-like cache")


def _check_quantiles(dh, V, burns):
    M = V.shape[-1]
    for n_burn in burns:
        with np.errstate(invalid="ignore"):
            want = np.quantile(V.reshape(-1, M)[n_burn:], Q, axis=0)
        got = dh.param_est_quantiles(n_burn, q=Q)
        assert got.shape == (3, M) and np.array_equal(got, want, equal_nan=True), (n_burn, got, want)


def _check_diagnostics(dh, V, n_burn, cols):
    N = V.shape[1]
    got, ref = dh.convergence_diagnostics(n_burn), reference(V, g0=-(-n_burn // N))
    assert got.r_hat.shape == got.ess.shape == (V.shape[-1],)
    cols = np.asarray(cols)
    print("r_hat rel. error", np.max(np.abs(got.r_hat[cols] / ref["r_hat"][cols] - 1.0)), "ess rel. error",
          np.max(np.abs(got.ess[cols] / ref["ess"][cols] - 1.0)), "margins", ref["margin"][cols].min())
    # 1e-10 is test_gpu_diagnostics' tolerance, set on columns at the origin.  Far from it the rounding of the half-chain means shows, in the
    # reference as on the device (and on an ordinary sampler as here).  u = 2^-53.  A mean of n values of size <= max |x| carries an error
    # <= (n - 1) u max |x| when summed in any order (the reference; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) and
    # <= 2 u max |x| when formed as shift + (sum of differences) / n (the device, diagnostics.h): eps = (n + 1) u max |x| between the two.
    # The deviations e_j of the m means from their mean move by <= 2 eps each (a common error of that mean cancels to second order, as does
    # the means' error in the within-chain variance W), so B = sum e_j^2 / (m - 1) moves by |dB| <= 4 eps sum |e_j| / (m - 1)
    # <= 4 eps sqrt(B m / (m - 1)) (Cauchy-Schwarz), and with r_hat^2 = (n - 1) / n + B / W >= (n - 1) / n
    #     |d r_hat| / r_hat = |dB| / (2 W r_hat^2) <= 2 eps sqrt(B m / (m - 1)) / W * n / (n - 1).
    # B and W are those of the window, restated here as in test_diagnostics_host.reference.  At the origin the term is below 1e-13; for an
    # output at 1e8 with unit spread and n = 17 it is about 1e-7.
    X = V[-(-n_burn // N):][:, :, cols]
    n = X.shape[0] // 2
    halves = np.concatenate([X[:n], X[X.shape[0] - n:]], axis=1)
    m = halves.shape[1]
    W, B = halves.var(axis=0, ddof=1).mean(axis=0), halves.mean(axis=0).var(axis=0, ddof=1)
    eps = (n + 1) * 2.0 ** -53 * np.abs(halves).max(axis=(0, 1))
    rtol = 1e-10 + 2.0 * eps * np.sqrt(B * m / (m - 1.0)) / W * n / (n - 1.0)
    err = np.abs(got.r_hat[cols] / ref["r_hat"][cols] - 1.0)
    print("largest r_hat error / bound", np.max(err / rtol), "largest bound", rtol.max(), "smallest bound", rtol.min())
    assert n == ref["n"] and m == ref["m"] and np.all(err <= rtol), (err, rtol)
    ok = cols[ref["margin"][cols] > 1e-6]                   # (a pair sum within rounding of zero could truncate either way)
    assert len(ok) >= 0.8 * len(cols)
    np.testing.assert_allclose(got.ess[ok], ref["ess"][ok], rtol=1e-8)
    assert np.array_equal(got.ess_capped[cols], ref["capped"][cols])


@pytest.fixture(scope="module")
def installed():
    X = _history_with_zero_denominators()
    G, N, d = X.shape
    e = _engine(N, d)
    e.set_history(X, X[-1])
    yield e, _over(e), e.get_loglike_history()
    e.close()


@pytest.fixture(scope="module")
def five(installed):
    e, s, LL = installed
    fn = _five()
    V = _values(s, fn)
    with s.derived_history(fn) as dh:
        yield dh, V, LL


def test_installed_history_values_padding_column_and_ln_likes(five):
    dh, V, LL = five
    assert V.shape == (40, 256, 5) and dh._engine.lib.bpm_abi_version() == 2
    _check_values(dh, V, LL)
    assert np.all(dh.param_est(0)[2][:, 4] == 0.0)                    # the output never written
    flat = V.reshape(-1, 5)
    assert np.isnan(flat[:, 0]).sum() == 1 and np.isposinf(flat[:, 0]).sum() >= 1 and np.isneginf(flat[:, 0]).sum() >= 1


def test_installed_history_quantiles(five):
    dh, V, _ = five
    _check_quantiles(dh, V, (0, 3, 256 * 5 + 1, 256 * 40 - 1))


def test_installed_history_histograms(five):
    dh, V, _ = five
    n_burn = 256 * 3 + 5
    W = V.reshape(-1, 5)[n_burn:]
    W2 = np.where(np.isnan(W), 1e300, W)                               # (for np.histogram2d: outside the range = counted nowhere)
    rng = [(1e8 / 0.7 - 5.0, 1e8 / 0.7 + 5.0), (-1.0, 8.0), (-8.0, 8.0)]
    ph = dh.param_est_hist(n_burn, bins=20, range=rng, dims=[0, 1, 3], pairs="all", bins2d=8)
    assert len(ph.pairs) == 3 and np.all(ph.counts.sum(axis=1) > len(W) // 2)        # (the ranges hold most values)
    with np.errstate(invalid="ignore"):
        TH.check_against_numpy(ph, W2, bins=20, rng=rng, bins2d=8)
        for j, k in enumerate(ph.dims):
            assert np.array_equal(ph.counts[j], np.histogram(W[:, k], 20, range=rng[j])[0])
    with pytest.raises(ValueError, match=r"autodetected range of \[nan, nan\] is not finite"):
        dh.param_est_hist(0, dims=[1])                                 # x0^2 + x4 carries x4's NaN
    with pytest.raises(ValueError, match=r"autodetected range of .* is not finite"):
        dh.param_est_hist(0)


def test_installed_history_covariance(five):
    dh, V, _ = five
    for n_burn in (0, 256 * 13 + 7):
        with np.errstate(invalid="ignore"):
            TC.check_against_numpy(dh.param_est_cov(n_burn), V.reshape(-1, 5)[n_burn:], long_double=True)


@pytest.mark.parametrize("every", [1, 7])
def test_installed_history_traces(five, every):
    dh, V, LL = five
    for n_burn in (0, 256 * 2 + 9):
        TT.check_against_numpy(dh.param_est_trace(n_burn, every=every, chains=[0, 17, 255]), V, LL, n_burn, every, chains=[0, 17, 255])


def test_a_function_of_derived_quantities(five):
    dh, V, LL = five
    fn2 = _pair()
    for n_burn in (0, 256 * 7 + 3):
        pd = dh.param_est_fn(fn2, n_burn, values=True)
        _check(pd, fn2, V, LL, n_burn, what=("of derived", n_burn))


@pytest.mark.parametrize("M", [1, 3, 256])
def test_layouts(installed, M):
    """n_out = 1: ld = 2, one output and one padding column; 3: odd, a tile that is no power of two; 256: the destination far wider than the
    source (d = 7).  Output m is x[m % 7] (m + 1): of the source's columns 0, 2 and 6 are finite and not constant."""
    e, s, LL = installed
    fn = _layout(M)
    V = _values(s, fn)
    with s.derived_history(fn) as dh:
        assert dh._engine.dim == M
        _check_values(dh, V, LL)
        _check_quantiles(dh, V, (0, 256 * 5 + 1, 256 * 40 - 1))
        _check_diagnostics(dh, V, 256 * 4 + 1, [m for m in range(M) if m % 7 in (0, 2, 6)])


def test_several_workgroups_ragged_last_tile_on_the_test_variant():
    from bipymc_amd import _lib as L
    N, d, G = 4096, 7, 64
    rs = np.random.RandomState(3)
    X = rs.normal(size=(G, N, d)) * np.arange(1, d + 1)
    X[:, :, 2] += 1e8
    X[10:12, 1000:3000, 4] = np.nan
    X[50, 4000, 0] = -np.inf
    e = _engine(N, d, lib=L.load_test())
    e.set_history(X, X[-1])
    s, fn = _over(e), _five()
    V = _values(s, fn)
    with s.derived_history(fn) as dh:
        assert dh._engine.lib is L.load_test() and dh._engine.lib is not L.load()
        _check_values(dh, V, e.get_loglike_history())
        _check_quantiles(dh, V, (N * 3 + 1,))
    e.close()


def _sampler_case(s, fn, n_burn):
    dh = s.derived_history(fn)                  # first: a history in position order must be put into chain order by this call itself
    try:
        V = _values(s, fn)
        _check_values(dh, V, s._engine.get_loglike_history())
        _check_quantiles(dh, V, (n_burn,))
    finally:
        dh.close()
    return V


def test_wide_rows_are_read_where_they_lie():
    from bipymc_amd import HipFunction
    s = _dream_class(64, 640, 30)
    _sampler_case(s, HipFunction(WIDE_SRC, n_out=3, params=[-2.0]), 64 * 2 + 1)


def test_dream_shuffled_history_in_position_order():
    s = _dream_class(256, 10, 60)
    _sampler_case(s, _five(), 256 * 4 + 9)


def test_serial_demc_and_a_function_with_exp():
    from bipymc_amd import HipFunction
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.3, dim=6)
    s = DeMc(t.ln_like, n_chains=64, seed=8)
    s.run_mcmc(64 * 100, np.zeros(6))
    V = _sampler_case(s, HipFunction(EXP_SRC, n_out=2), 64 * 5 + 1)
    W = s.param_est(0)[2]
    assert np.allclose(V.reshape(-1, 2)[:, 0], np.exp(-0.5 * W[:, 0] * W[:, 0]), rtol=1e-12, atol=0.0)
    _bits_equal(V.reshape(-1, 2)[:, 1], W[:, 2] / W[:, 1], "the arithmetic output")


def test_snapshot_and_no_side_effects():
    fn = _five()

    def start():
        e = _engine(256, 12)
        e.set_state(np.random.RandomState(1).normal(size=(256, 12)))
        e.begin_run()
        e.step(100)
        return e

    a, b = start(), start()
    s = _over(a)
    dh = s.derived_history(fn)
    assert dh.history_rows == 101
    q1, d1 = dh.param_est_quantiles(256 * 3 + 9, q=Q), dh.convergence_diagnostics(256 * 10)
    V1 = dh.param_est(0)[2].copy()
    a.step(100)
    b.step(100)
    q2, d2 = dh.param_est_quantiles(256 * 3 + 9, q=Q), dh.convergence_diagnostics(256 * 10)
    assert np.array_equal(q1.view(np.uint64), q2.view(np.uint64))
    for f in ("r_hat", "ess"):
        assert np.array_equal(getattr(d1, f).view(np.uint64), getattr(d2, f).view(np.uint64)), f
    assert dh.history_rows == 101 and np.array_equal(dh.param_est(0)[2].view(np.uint64), V1.view(np.uint64))
    assert np.array_equal(a.get_history(), b.get_history())
    assert np.array_equal(a.get_loglike_history(), b.get_loglike_history())
    assert np.array_equal(a.get_state(), b.get_state())
    assert np.array_equal(a.get_loglike(), b.get_loglike())
    with s.derived_history(fn) as later:
        assert later.history_rows == 201
        _bits_equal(later.param_est(0)[2][:256 * 101], V1, "the first 101 generations")
    dh.close()
    dh.close()
    for call in (lambda: dh.param_est_quantiles(0), lambda: dh.convergence_diagnostics(0), lambda: dh.param_est(0)):
        with pytest.raises(RuntimeError, match="this derived history is closed"):
            call()
    a.close()
    b.close()


def test_errors_name_what_is_wrong():
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    fn = _five()
    e = _engine(64, 5, burnin_gen=0, keep_history=False)
    e.set_state(np.zeros((64, 5)) + np.arange(5))
    e.begin_run()
    e.step(10)
    with pytest.raises(L.BpmError, match="bpm_derive_history: needs keep_history=True"):
        e.derive_history(fn)
    e.close()
    e = _engine(64, 5)
    e.set_state(np.random.RandomState(2).normal(size=(64, 5)))
    e.begin_run()
    e.step(20)

    def dest(**kw):
        args = dict(algo=L.ALGO_DEMC, n_chains=64, dim=5, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=0, burnin_gen=0)
        args.update(kw)
        return HipEngine(**args)

    def call(src, dst):
        src._ck(src.lib.bpm_derive_history(src._h, dst._h))

    good = dest()
    with pytest.raises(L.BpmError, match=r"bpm_derive_history: no device function installed on the source \(bpm_set_device_function\)"):
        call(e, good)
    e.set_device_function(FIVE_SRC, 5, [0.25, -3.0])
    with pytest.raises(L.BpmError, match="bpm_derive_history: the destination is the source itself"):
        call(e, e)
    with pytest.raises(L.BpmError, match="bpm_derive_history: null handle"):
        e._ck(e.lib.bpm_derive_history(e._h, None))
    for kw, text in ((dict(dim=6), "bpm_derive_history: the destination has dim 6; the installed function has n_out 5"),
                     (dict(n_chains=32), "bpm_derive_history: the destination has n_chains 32; the source has 64"),
                     (dict(keep_history=False), "bpm_derive_history: the destination needs keep_history=True")):
        bad = dest(**kw)
        with pytest.raises(L.BpmError, match=text):
            call(e, bad)
        bad.close()
    from bipymc_amd.utils import d100_gauss
    tid, tp, _ = d100_gauss.Gauss_100D(rho=0.5, dim=5)._bpm_target_spec()
    bad = dest(target_id=tid, target_params=tp)
    with pytest.raises(L.BpmError, match="bpm_derive_history: the destination must have the host-callback target"):
        call(e, bad)
    bad.close()
    call(e, good)                                                      # ... and the same handles, in order, work
    assert good.history_rows() == 21
    _bits_equal(good.get_history().reshape(-1, 5), _over(e).param_est_fn(fn, 0, values=True).values)
    good.close()
    with pytest.raises(TypeError, match="derived_history: fn must be a HipFunction"):
        _over(e).derived_history(FIVE_SRC)
    e.close()
    from bipymc_amd.samplers import DeMc
    with pytest.raises(RuntimeError, match="derived_history: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).derived_history(fn)
