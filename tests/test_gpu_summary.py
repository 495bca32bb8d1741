"""The posterior summary on the GPU (bpm_hdi and bpm_rank_history kind 5, bipymc_amd/csrc/ranks.h + bipymc_amd/summary.py) against the NumPy
restatement of tests/_summary_restatement.py.

Tolerances.
  HDI, order statistics, median, quantiles, NaN counts, the squared-deviation fill     exact (np.array_equal, NaN-equal; the fill bit for bit:
               (x - c) * (x - c) is the two IEEE operations of NumPy's (x - c) ** 2).
  R-hat / ESS (r_hat, r_hat_classic, ess_bulk, ess_tail, ess_mean, ess_sd)     the project's criteria (tests/_rank_restatement.check_diagnostics):
               r_hat 1e-10 relative; ess 1e-8 relative where the pair sum that ended Geyer's sequence is further than 1e-6 from zero, which must
               hold for at least 80 % of the coordinates that are not NaN.
  mean, sd, mcse_mean, mcse_sd     what follows from those and from the sums' rounding bounds: tests/_summary_restatement.py (mean_atol, sd_rtol,
               mcse_mean_rtol, mcse_sd_rtol), derived in tests/test_summary_host.py::test_gpu_tolerances_follow_from_the_formats."""
import gc
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _rank_restatement as RR  # noqa: E402
import _summary_restatement as SR  # noqa: E402
from _history_cases import _engine  # noqa: E402
from test_diagnostics_host import _ar1  # noqa: E402
from test_gpu_rank_diagnostics import D, G, N, _bits, _free_device_memory, _over, _tied_history  # noqa: E402

PROBS = (0.94, 0.5, 1e-5)
N_BURN_PARTIAL = 64 * 100 + 17        # a partial first generation: chains 17 ... 63 of history row 100


@pytest.fixture(scope="module")
def tied():
    X = _tied_history()
    e = _engine(N, D)
    e.set_history(X, X[-1])
    yield e, _over(e), X
    e.close()


def _same(got, want):
    return np.array_equal(got, want, equal_nan=True)


def _check_hdi(got, flat, probs):
    """got: (lo, hi, n_nan, S) of the device; flat (S, d): the window's values"""
    lo, hi, n_nan = SR.hdi_columns(flat, probs)
    assert got[3] == len(flat)
    assert _same(got[0], lo) and _same(got[1], hi), (got[0], lo, got[1], hi)
    assert np.array_equal(got[2], n_nan)


def test_hdi_is_exact_over_both_windows_whatever_the_batch(tied, monkeypatch):
    e, s, X = tied
    split = RR.split_rows(X).reshape(-1, D)
    S = len(split)
    assert S == 25600
    # the first-index rule is exercised: a column of this history has many indices of the smallest width
    srt = np.sort(split[:, 1])
    w = srt[SR.hdi_offset(0.5, S):] - srt[:S - SR.hdi_offset(0.5, S)]
    assert (w == w.min()).sum() > 1
    # ... and at m = 0 the column with -inf has a NaN width at index 0
    lo, hi, _ = SR.hdi_columns(split, [1e-5])
    assert lo[0, 3] == -np.inf and hi[0, 3] == -np.inf
    pos = [0, 1, S // 2, S - 1]
    first = {}
    for batch in ("2", None):                                    # three batches with the last partial, then the default batch
        if batch is None:
            monkeypatch.delenv("BPM_RANK_BATCH_COLS")
        else:
            monkeypatch.setenv("BPM_RANK_BATCH_COLS", batch)
        got = e.hdi(0, 0, G, PROBS, pos)
        _check_hdi(got, split, PROBS)
        assert np.array_equal(got[4], np.sort(split, axis=0)[pos])
        one = s.param_est_hdi(prob=0.94)
        assert one.lo.shape == (D,) and one.n == G * N and one.prob == 0.94
        _check_hdi((one.lo[None], one.hi[None], one.n_nan, one.n), SR.param_est_window(X, 0), [0.94])
        for n_burn in (0, N_BURN_PARTIAL):
            h = s.param_est_hdi(n_burn=n_burn, prob=PROBS)
            assert h.lo.shape == (3, D)
            _check_hdi((h.lo, h.hi, h.n_nan, h.n), SR.param_est_window(X, n_burn), PROBS)
            key = ("param_est", n_burn)
            if key in first:
                assert np.array_equal(_bits(h.lo), _bits(first[key].lo)) and np.array_equal(_bits(h.hi), _bits(first[key].hi))
            first.setdefault(key, h)
        if "split" in first:
            assert np.array_equal(_bits(got[0]), _bits(first["split"][0])) and np.array_equal(_bits(got[1]), _bits(first["split"][1]))
        first.setdefault("split", got)


def _small_history(N_, G_, d, seed):
    rs = np.random.RandomState(seed)
    X = np.round(rs.normal(size=(G_, N_, d)) * 3.0, 1)            # one decimal: ties, also in the widths
    X[X == 0.0] = -0.0
    return X


@pytest.mark.parametrize("N_,G_,d,probs,n_burns", [
    (4, 9, 1, (0.94, 0.5, 0.03), (0, 4 * 2 + 1, 4 * 8 + 3)),      # S = 32 split, 36 / 27 / 1 param_est: fewer values than a workgroup has lanes; ld = 2
    (7, 40, 3, (0.5, 0.505, 0.94), (0, 7 * 3 + 4, 7 * 3 + 5)),    # n_local odd: column offsets and e0 of both parities; m = 140 and 141
    (8, 12, 600, (0.9, 0.2), (0, 8 * 5 + 3)),                     # a wide row: 600 columns, several tiles of the keys kernel
])
def test_smallest_shapes(N_, G_, d, probs, n_burns):
    X = _small_history(N_, G_, d, seed=N_)
    if d == 3:
        X[5, 2, 1] = np.nan
        X[6, 1, 2], X[30, 4, 2] = np.inf, np.inf
        split_S = 2 * (G_ // 2) * N_
        assert [SR.hdi_offset(p, split_S) % 2 for p in probs[:2]] == [0, 1]
    e = _engine(N_, d)
    try:
        e.set_history(X, X[-1])
        s = _over(e)
        _check_hdi(e.hdi(0, 0, G_, probs), RR.split_rows(X).reshape(-1, d), probs)
        _check_hdi(e.hdi(0, 1, G_ - 1, probs), RR.split_rows(X[:G_ - 1], 1).reshape(-1, d), probs)
        for n_burn in n_burns:
            h = s.param_est_hdi(n_burn=n_burn, prob=probs)
            _check_hdi((h.lo, h.hi, h.n_nan, h.n), SR.param_est_window(X, n_burn), probs)
    finally:
        e.close()


def test_demc_banana_shuffled_history_with_snooker():
    from bipymc_amd.demc import DeMcMpi
    from bipymc_amd.utils import banana_rv
    s = DeMcMpi(banana_rv.Banana_2D().ln_like, np.zeros(2), n_chains=512, seed=99, p_snooker=0.2)
    s.run_mcmc(512 * 400)
    n_burn = 512 * 100 + 5
    h = s.param_est_hdi(n_burn=n_burn, prob=(0.94, 0.5))         # first: a history in position order is put into chain order by this call
    H = s._engine.get_history()
    _check_hdi((h.lo, h.hi, h.n_nan, h.n), SR.param_est_window(H, n_burn), (0.94, 0.5))
    assert np.array_equal(SR.param_est_window(H, n_burn), s.param_est(n_burn)[2])
    got = s.posterior_summary(n_burn=n_burn)
    assert got.window == (101, 400)
    SR.check_summary(got, H, g0=101)


def test_a_derived_history_of_three_outputs(tied):
    from bipymc_amd import HipFunction
    e, s, X = tied
    fn = HipFunction("""
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[0] + x[4]; out[1] = x[1] * p[0]; out[2] = x[0] * x[0];
}""", n_out=3, params=[0.5])
    with s.derived_history(fn) as dh:
        V = dh._engine.get_history()
        h = dh.param_est_hdi(n_burn=N * 3 + 1, prob=PROBS)
        got = dh.posterior_summary(n_burn=N * 3 + 1)
    _check_hdi((h.lo, h.hi, h.n_nan, h.n), SR.param_est_window(V, N * 3 + 1), PROBS)
    SR.check_summary(got, V, g0=4)


def test_squared_deviation_fill_is_numpys_bit_for_bit(tied):
    """kind 5 of bpm_rank_history.  The padding column of this odd dim cannot be read back through the ABI (bpm_get_history copies dim
    columns); what reads whole rows of ld doubles can: the covariance's matrix-core SYRK over the filled handle equals np.cov of the fill."""
    from bipymc_amd import _lib as L
    from bipymc_amd.derived import DerivedHistory
    from bipymc_amd.comm import single_process_allgather
    e, s, X = tied
    W = RR.split_rows(X, 21)
    c = np.array([0.25, -1.0, 0.0, 1e300, np.mean(W[:, :, 4])])
    dst, os_ = e.rank_history(21, G, 5, c)
    try:
        assert os_.shape == (0, D) and dst.history_rows() == W.shape[0]
        with np.errstate(invalid="ignore", over="ignore"):
            want = (W - c) ** 2
        assert np.array_equal(_bits(dst.get_history()), _bits(want))
        LL = e.get_loglike_history()
        n = W.shape[0] // 2
        assert np.array_equal(_bits(dst.get_loglike_history()), _bits(np.concatenate([LL[21:21 + n], LL[G - n:]])))
        cov = DerivedHistory(dst, N, single_process_allgather).param_est_cov()
        np.testing.assert_allclose(cov.cov[np.ix_([0, 1, 2, 4], [0, 1, 2, 4])], np.cov(want.reshape(-1, D)[:, [0, 1, 2, 4]], rowvar=False), rtol=1e-9)
        e.rank_history(21, G, 3, c, (), dst)                          # ... and the same handle is filled again, by another kind and back
        e.rank_history(21, G, 5, c, (), dst)
        assert np.array_equal(_bits(dst.get_history()), _bits(want))
    finally:
        dst.close()
    with pytest.raises(L.BpmError, match="bpm_rank_history: kind 5 needs arg"):
        e.rank_history(0, G, 5)
    with pytest.raises(L.BpmError, match=r"bpm_rank_history: the squared deviation sorts nothing and has no order statistics \(n_pos must be 0\)"):
        e.rank_history(0, G, 5, c, [0])
    with pytest.raises(L.BpmError, match=r"bpm_rank_history: kind must be 0 \(rank\), .* or 5 \(squared deviation\); got 6"):
        e.rank_history(0, G, 6, c)


def test_posterior_summary_on_the_tied_history(tied):
    e, s, X = tied
    got = s.posterior_summary()
    print(got)
    f = SR.check_summary(got, X)
    # the four coordinates without +-inf are live in every column
    live = [0, 1, 2, 4]
    for name in ("mean", "sd", "mcse_mean", "mcse_sd", "ess_mean", "ess_sd", "ess_bulk", "ess_tail", "r_hat", "r_hat_classic", "hdi_lo", "hdi_hi"):
        assert np.isfinite(getattr(got, name)[live]).all(), name
    assert (f["ref_mean"]["margin"][live] > SR.ESS_MARGIN).all() and (f["ref_sd"]["margin"][live] > SR.ESS_MARGIN).all()
    assert len(str(got).splitlines()) == D + 2
    got = s.posterior_summary(n_burn=N * 20 + 7, hdi_prob=0.5, prob=(0.1, 0.75), max_lag=5)
    SR.check_summary(got, X, g0=21, hdi_prob=0.5, prob=(0.1, 0.75), max_lag=5)
    assert got.window == (21, G) and got.ess_capped.any()


def test_posterior_summary_on_an_ar1_history():
    phis = [0.0, 0.5, 0.9, 0.5, 0.0]
    X = _ar1(401, 64, phis, seed=11, offset=np.array([0.0, 10.0, -3.0, 0.0, 1e3]))
    e = _engine(64, 5)
    e.set_history(X, X[-1])
    got = _over(e).posterior_summary()
    e.close()
    SR.check_summary(got, X)
    # an AR(1) chain's ESS per draw is (1 - phi) / (1 + phi); the standard error of its mean grows by the root of the inverse
    assert got.ess_mean[2] < 0.2 * got.ess_mean[0] and got.mcse_mean[2] / got.sd[2] > 2.0 * got.mcse_mean[0] / got.sd[0]
    assert (got.hdi_lo < got.median).all() and (got.median < got.hdi_hi).all()


def test_no_side_effects_and_no_leak():
    def start():
        e = _engine(256, 12)
        e.set_state(np.random.RandomState(1).normal(size=(256, 12)))
        e.begin_run()
        e.step(100)
        return e

    a, b = start(), start()
    s = _over(a)
    n_burn = 256 * 3 + 9
    rows = a.history_rows()
    r1, h1 = s.posterior_summary(n_burn=n_burn), s.param_est_hdi(n_burn=n_burn)      # (also loads whatever the first call loads)
    for eng in (a, b):                                               # a quantile and a trace window open on both
        assert eng.quantile_begin(n_burn) == rows * 256 - n_burn
        eng.trace_bins(4, rows, 10)
    gc.collect()                                                     # (tests/test_gpu_rank_diagnostics.py: test_no_side_effects_and_no_leak)
    free0 = _free_device_memory()
    r2, h2 = s.posterior_summary(n_burn=n_burn), s.param_est_hdi(n_burn=n_burn)
    assert _free_device_memory() == free0                            # the scratch handle, the sort's scratch and the scan's partials are gone
    assert a.history_rows() == rows
    for f in ("mean", "sd", "hdi_lo", "hdi_hi", "median", "quantiles", "mcse_mean", "mcse_sd", "ess_mean", "ess_sd", "ess_bulk", "ess_tail", "r_hat"):
        assert np.array_equal(_bits(getattr(r1, f)), _bits(getattr(r2, f))), f
    assert np.array_equal(_bits(h1.lo), _bits(h2.lo)) and np.array_equal(_bits(h1.hi), _bits(h2.hi))
    # the open windows still answer, and as on the engine nothing was asked of
    pk, pv = np.zeros(12, dtype=np.int32) + np.arange(12, dtype=np.int32), np.zeros(12, dtype=np.uint64)
    qa, qb = a.quantile_histogram(pk, pv, 0), b.quantile_histogram(pk, pv, 0)
    assert np.array_equal(qa[0], qb[0]) and np.array_equal(qa[1], qb[1])
    ta, tb = a.trace_chains([0, 255]), b.trace_chains([0, 255])
    assert np.array_equal(ta[1], tb[1]) and np.array_equal(ta[2], tb[2])
    a.step(100)
    b.step(100)
    assert np.array_equal(a.get_history(), b.get_history()) and np.array_equal(a.get_loglike_history(), b.get_loglike_history())
    assert np.array_equal(a.get_state(), b.get_state()) and np.array_equal(a.get_loglike(), b.get_loglike())
    a.close()
    b.close()


def test_errors_name_what_is_wrong(monkeypatch):
    from bipymc_amd import _lib as L
    e = _engine(64, 5, burnin_gen=0, keep_history=False)
    e.set_state(np.zeros((64, 5)) + np.arange(5))
    e.begin_run()
    e.step(10)
    with pytest.raises(L.BpmError, match="bpm_hdi: needs keep_history=True"):
        _over(e).param_est_hdi()
    with pytest.raises(L.BpmError, match="needs keep_history=True"):
        _over(e).posterior_summary()
    e.close()
    e = _engine(64, 1)
    X = np.random.RandomState(3).normal(size=(1030, 64, 1))
    e.set_history(X, X[-1])
    s = _over(e)
    for p, text in ((0.0, "bpm_hdi: probability 0.000000 is outside \\(0, 1\\)"), (1.0, "bpm_hdi: probability 1.000000 is outside \\(0, 1\\)"),
                    (np.nan, "bpm_hdi: probability -?nan is outside \\(0, 1\\)")):
        with pytest.raises(L.BpmError, match=text):
            e.hdi(1, 0, 0, [0.5, p])
        with pytest.raises(ValueError, match=r"param_est_hdi: every probability must lie inside \(0, 1\)"):
            s.param_est_hdi(prob=p)
        with pytest.raises(ValueError, match=r"posterior_summary: every probability must lie inside \(0, 1\)"):
            s.posterior_summary(hdi_prob=p)
    with pytest.raises(L.BpmError, match=r"bpm_hdi: n_prob = 9 is outside the supported 1 \.\.\. 8 probabilities per call"):
        e.hdi(1, 0, 0, [0.1] * 9)
    with pytest.raises(L.BpmError, match=r"bpm_hdi: n_prob = 0 is outside the supported 1 \.\.\. 8"):
        e.hdi(1, 0, 0, [])
    with pytest.raises(ValueError, match="param_est_hdi: 9 probabilities given; one call takes 1 ... 8"):
        s.param_est_hdi(prob=[0.1] * 9)
    with pytest.raises(L.BpmError, match=r"bpm_hdi: the window is empty \(n_burn = 65920 is at or beyond the last super-chain row\)"):
        e.hdi(1, 1030 * 64, 0, [0.5])
    with pytest.raises(ValueError, match=r"param_est_hdi: the window is empty \(n_burn = 65920"):
        s.param_est_hdi(n_burn=1030 * 64)
    with pytest.raises(L.BpmError, match=r"bpm_hdi: the window is empty \(1 history rows give half-chains of no draws\)"):
        e.hdi(0, 5, 6, [0.5])
    with pytest.raises(L.BpmError, match="bpm_hdi: generation range out of bounds"):
        e.hdi(0, 5, 1031, [0.5])
    with pytest.raises(L.BpmError, match="bpm_hdi: window must be 0 .* or 1 .*; got 2"):
        e.hdi(2, 0, 0, [0.5])
    with pytest.raises(L.BpmError, match=r"bpm_hdi: order statistic 65920 is outside \[0, 65920\)"):
        e.hdi(1, 0, 0, [0.5], [65920])
    with pytest.raises(L.BpmError, match="at least 4 are needed"):
        s.posterior_summary(n_burn=64 * 1024)
    monkeypatch.setenv("BPM_RANK_SCRATCH_MB", "1")                 # one column of 65920 keys is 1 054 720 bytes of keys alone
    with pytest.raises(L.BpmError, match=r"bpm_hdi: sorting one column of 65920 keys needs \d+ bytes of scratch \(keys in, keys out and the "
                                         r"sort's temporaries\); the budget is 1048576 bytes"):
        s.param_est_hdi()
    with pytest.raises(L.BpmError, match=r"bpm_hdi: sorting one column of 65920 keys needs \d+ bytes of scratch"):
        s.posterior_summary()
    monkeypatch.delenv("BPM_RANK_SCRATCH_MB")
    h = s.param_est_hdi(prob=0.5)                                      # ... and the same engine, in order, works
    _check_hdi((h.lo[None], h.hi[None], h.n_nan, h.n), X.reshape(-1, 1), [0.5])
    e.close()
    from bipymc_amd.samplers import DeMc
    with pytest.raises(RuntimeError, match="posterior_summary: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).posterior_summary()
    with pytest.raises(RuntimeError, match="param_est_hdi: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).param_est_hdi()
