"""Rank-normalized diagnostics on the GPU (bpm_rank_history, bipymc_amd/csrc/ranks.h + bipymc_amd/rank_diagnostics.py) against the NumPy / SciPy
restatement of tests/_rank_restatement.py (rankdata(method="average"), ndtri, np.median, np.quantile, then tests/test_diagnostics_host.reference
of each transformed array).

Tolerances.
  ranks, order statistics, median, quantiles, indicators     exact (np.array_equal).
  z scores     rtol = Z_RTOL.  The argument of Phi^-1, (r - 3/8) / (S + 1/4), is the same double on both sides -- r is a half-integer below
               2^32, r - 3/8 and S + 1/4 are exact, the quotient is one correctly rounded division here and there -- so the only difference
               is the device's normcdfinv against SciPy's ndtri.  MEASURED on an MI355X over this file's grid (every half-integer rank that
               occurs in _tied_history(), S = 25600, both plain and folded): largest relative difference Z_MEASURED = 8.882e-16
               (test_z_scores prints it), far below the 1e-13 above which a bug would have been looked for first.  Z_RTOL = 4 x Z_MEASURED
               = 3.6e-15: the margin is there because the grid moves with S.
  R-hat / ESS  the project's criteria (tests/test_gpu_diagnostics.py): r_hat 1e-10 relative; ess 1e-8 relative where the pair sum that ended
               Geyer's sequence is further than 1e-6 from zero, which must hold for at least 80 % of the coordinates; capped equal."""
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
from _history_cases import _dream_class, _engine, _over  # noqa: E402
from test_diagnostics_host import _ar1  # noqa: E402

Z_MEASURED = 8.882e-16     # (plain 8.882e-16 over 16473 distinct arguments, folded 7.772e-16 over 16548: four units of 2^-52)
Z_RTOL = 4 * Z_MEASURED
N, G, D = 64, 401, 5       # G odd: the middle row is dropped; d odd: ld = 6, one padding column


def _tied_history():
    """Metropolis-like ties: 80 % of every chain's rows repeat the previous row; coordinate 1 rounded to integers, coordinate 2 a mixture of
    -0.0 and +0.0 among other values, coordinate 3 with a few +-inf"""
    rs = np.random.RandomState(4)
    X = rs.normal(size=(G, N, D)) * np.array([1.0, 3.0, 1.0, 2.0, 0.5])
    stay = rs.uniform(size=(G, N)) < 0.8
    for g in range(1, G):
        X[g][stay[g]] = X[g - 1][stay[g]]
    X[:, :, 1] = np.round(X[:, :, 1])
    c2 = X[:, :, 2]
    c2[np.abs(c2) < 0.4] = np.where(c2[np.abs(c2) < 0.4] < 0, -0.0, 0.0)
    X[7, 3, 3], X[300, 60, 3], X[301, 60, 3], X[150, 9, 3] = np.inf, -np.inf, -np.inf, np.inf
    assert np.signbit(c2[c2 == 0]).any() and not np.signbit(c2[c2 == 0]).all()
    return X


@pytest.fixture(scope="module")
def tied():
    X = _tied_history()
    e = _engine(N, D)
    e.set_history(X, X[-1])
    yield e, _over(e), X, RR.restate(X)
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_ranks_are_exact_whatever_the_batch(tied, monkeypatch):
    e, s, X, t = tied
    n = G // 2
    with s.rank_history(scale="rank") as rh:
        assert (rh.history_rows, rh.n_chains, rh.dim) == (2 * n, N, D)
        r1 = rh._engine.get_history()
        assert np.array_equal(r1, t["rank"])
        assert np.array_equal(r1 * 2, np.round(r1 * 2)) and r1.min() >= 1.0 and r1.max() <= 2 * n * N
        # the handle is what bpm_set_history leaves: the ln-likes of the same generations, the state = the last row
        LL = e.get_loglike_history()
        assert np.array_equal(_bits(rh._engine.get_loglike_history()), _bits(np.concatenate([LL[:n], LL[G - n:]])))
        assert np.array_equal(rh._engine.get_state(), r1[-1]) and np.array_equal(_bits(rh._engine.get_loglike()), _bits(LL[-1]))
        assert np.array_equal(rh.param_est_quantiles(0, q=(0.5,))[0], np.quantile(r1.reshape(-1, D), 0.5, axis=0))
    with s.rank_history(scale="rank", folded=True) as rh:
        f1 = rh._engine.get_history()
        assert np.array_equal(f1, t["rank_folded"])
    monkeypatch.setenv("BPM_RANK_BATCH_COLS", "2")       # three batches, the last partial
    with s.rank_history(scale="rank") as rh:
        assert np.array_equal(_bits(rh._engine.get_history()), _bits(r1))
    with s.rank_history(scale="rank", folded=True) as rh:
        assert np.array_equal(_bits(rh._engine.get_history()), _bits(f1))
    with s.rank_history(scale="z") as rh:
        z2 = rh._engine.get_history()
    monkeypatch.delenv("BPM_RANK_BATCH_COLS")
    with s.rank_history(scale="z") as rh:
        assert np.array_equal(_bits(rh._engine.get_history()), _bits(z2))


def test_z_scores(tied):
    e, s, X, t = tied
    worst = 0.0
    for folded, name in ((False, "bulk"), (True, "folded")):
        with s.rank_history(scale="z", folded=folded) as rh:
            z = rh._engine.get_history()
        want = t[name]
        assert np.isfinite(want).all() and np.array_equal(z == 0.0, want == 0.0)
        nz = want != 0.0
        rel = float(np.max(np.abs(z[nz] / want[nz] - 1.0)))
        print("normcdfinv against ndtri, %s: largest relative difference %.3e over %d distinct arguments" % (name, rel, len(np.unique(want))))
        worst = max(worst, rel)
        np.testing.assert_allclose(z, want, rtol=Z_RTOL, atol=0.0)
    print("largest relative difference of the z scores: %.3e (Z_RTOL = %.3e)" % (worst, Z_RTOL))


def test_order_statistics_median_and_quantiles_are_numpys(tied):
    e, s, X, t = tied
    flat = t["split"].reshape(-1, D)
    S = len(flat)
    pos = [0, 1, S // 20, S // 2 - 1, S // 2, S - 2, S - 1]
    dst, os_ = e.rank_history(0, G, 0, None, pos)
    dst.close()
    assert np.array_equal(os_, np.sort(flat, axis=0)[pos])
    med = np.median(np.abs(flat - t["median"]), axis=0)
    dst, os_ = e.rank_history(0, G, 2, t["median"], [S // 2 - 1, S // 2])
    dst.close()
    assert np.array_equal(os_.mean(axis=0), med)
    got = s.convergence_diagnostics_rank(prob=(0.1, 0.75))
    assert np.array_equal(got.median, t["median"]) and np.array_equal(got.quantiles, np.quantile(flat, (0.1, 0.75), axis=0))


def test_diagnostics_on_the_tied_history(tied):
    e, s, X, t = tied
    got = s.convergence_diagnostics_rank()
    RR.check_diagnostics(got, X)
    assert np.isfinite(got.r_hat).all() and np.isfinite(got.ess_tail).all()
    got = s.convergence_diagnostics_rank(n_burn=N * 20 + 7, max_lag=5)
    RR.check_diagnostics(got, X, g0=21, max_lag=5)
    assert got.window == (21, G) and got.ess_capped.any()


def test_diagnostics_on_an_ar1_history():
    X = _ar1(401, 64, [0.0, 0.5, 0.9, 0.5, 0.0], seed=11)
    e = _engine(64, 5)
    e.set_history(X, X[-1])
    got = _over(e).convergence_diagnostics_rank()
    e.close()
    RR.check_diagnostics(got, X)
    # an AR(1) chain's ESS per draw is (1 - phi) / (1 + phi): 1 at phi = 0, 0.053 at phi = 0.9; normal scores of a Gaussian keep that order
    assert got.ess_bulk[2] < 0.2 * got.ess_bulk[0]


def test_chains_that_differ_in_scale_are_seen_by_the_folded_r_hat_only():
    """the restatement gives classic 1.0004 / 1.005 / 0.9999 against r_hat_tail 1.152 / 1.150 / 1.152"""
    X = _ar1(401, 64, [0.0, 0.5, 0.0], seed=5)
    X[:, :32, :] *= 3.0
    e = _engine(64, 3)
    e.set_history(X, X[-1])
    s = _over(e)
    classic, got = s.convergence_diagnostics(), s.convergence_diagnostics_rank()
    e.close()
    print("classic", classic.r_hat, "bulk", got.r_hat_bulk, "tail", got.r_hat_tail)
    assert (classic.r_hat[[0, 2]] < 1.01).all()
    assert (got.r_hat_tail > 1.1).all() and np.array_equal(got.r_hat, got.r_hat_tail)
    RR.check_diagnostics(got, X)


def test_degenerate_coordinates():
    X = _ar1(81, 64, [0.5, 0.5, 0.5, 0.5], seed=2)
    clean = X.copy()
    X[:, :, 1] = 2.5
    X[7, 3, 2] = np.nan
    e = _engine(64, 4)
    e.set_history(X, X[-1])
    got = _over(e).convergence_diagnostics_rank()
    with _over(e).rank_history(scale="rank") as rh:
        r = rh._engine.get_history()
    e.set_history(clean, clean[-1])
    ref = _over(e).convergence_diagnostics_rank()
    e.close()
    RR.check_diagnostics(got, X)
    assert np.isnan(r[:, :, 2]).all() and np.all(r[:, :, 1] == (80 * 64 + 1) / 2.0) and np.isfinite(r[:, :, [0, 3]]).all()
    for name in RR.FIELDS:
        f = getattr(got, name)
        assert np.isnan(f[[1, 2]]).all() and np.array_equal(_bits(f[[0, 3]]), _bits(getattr(ref, name)[[0, 3]])), name
    assert got.median[1] == 2.5 and np.isnan(got.median[2]) and np.isnan(got.quantiles[:, 2]).all()


def _sampler_case(s, n_burn):
    got = s.convergence_diagnostics_rank(n_burn=n_burn)      # first: a history in position order is put into chain order by this call
    H = s._engine.get_history()
    g0 = -(-n_burn // s.n_chains)
    t = RR.check_diagnostics(got, H, g0=g0)
    with s.rank_history(n_burn=n_burn, scale="rank") as rh:
        assert np.array_equal(rh._engine.get_history(), t["rank"])
    return got


def test_demc_banana_shuffled_history_with_snooker():
    from bipymc_amd.demc import DeMcMpi
    from bipymc_amd.utils import banana_rv
    s = DeMcMpi(banana_rv.Banana_2D().ln_like, np.zeros(2), n_chains=512, seed=99, p_snooker=0.2)
    s.run_mcmc(512 * 400)
    got = _sampler_case(s, 512 * 100 + 5)
    assert got.window == (101, 400)                            # (row 0 is the initial state: 400 rows)


def test_wide_rows():
    _sampler_case(_dream_class(64, 640, 150), 64 * 10)


def test_serial_demc():
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.3, dim=6)
    s = DeMc(t.ln_like, n_chains=64, seed=8)
    s.run_mcmc(64 * 300, np.zeros(6))
    _sampler_case(s, 64 * 50 + 1)


def test_a_derived_history_of_three_outputs(tied):
    from bipymc_amd import HipFunction
    e, s, X, t = tied
    fn = HipFunction("""
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[0] + x[4]; out[1] = x[1] * p[0]; out[2] = x[0] * x[0];
}""", n_out=3, params=[0.5])
    with s.derived_history(fn) as dh:
        V = dh._engine.get_history()
        assert np.array_equal(V, np.stack([X[:, :, 0] + X[:, :, 4], X[:, :, 1] * 0.5, X[:, :, 0] * X[:, :, 0]], axis=2))
        got = dh.convergence_diagnostics_rank(n_burn=N * 3 + 1)
    RR.check_diagnostics(got, V, g0=4)


def _free_device_memory():
    """hipMemGetInfo of the runtime the library runs on (the engines' calls end in a synchronise)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_no_side_effects_and_no_leak():
    def start():
        e = _engine(256, 12)
        e.set_state(np.random.RandomState(1).normal(size=(256, 12)))
        e.begin_run()
        e.step(100)
        return e

    a, b = start(), start()
    s = _over(a)
    r1 = s.convergence_diagnostics_rank(n_burn=256 * 3 + 9)          # (also loads whatever the first call loads)
    # earlier tests' sampler objects refer to themselves (DeMc / DeMcMpi: _frozen_ln_like_fn) and give their device memory back only when the cycle
    # collector runs: it runs HERE, not at some allocation between the two readings, where the memory it frees would look like a negative leak
    gc.collect()
    free0 = _free_device_memory()
    r2 = s.convergence_diagnostics_rank(n_burn=256 * 3 + 9)
    with s.rank_history(n_burn=256 * 3 + 9, folded=True):
        pass
    assert _free_device_memory() == free0                      # the scratch handle and the sort's scratch are gone
    for f in RR.FIELDS + ("median", "quantiles"):
        assert np.array_equal(_bits(getattr(r1, f)), _bits(getattr(r2, f))), f
    a.step(100)
    b.step(100)
    assert np.array_equal(a.get_history(), b.get_history()) and np.array_equal(a.get_loglike_history(), b.get_loglike_history())
    assert np.array_equal(a.get_state(), b.get_state()) and np.array_equal(a.get_loglike(), b.get_loglike())
    a.close()
    b.close()


def test_errors_name_what_is_wrong(monkeypatch):
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    e = _engine(64, 5, burnin_gen=0, keep_history=False)
    e.set_state(np.zeros((64, 5)) + np.arange(5))
    e.begin_run()
    e.step(10)
    with pytest.raises(L.BpmError, match="bpm_rank_history: needs keep_history=True"):
        _over(e).convergence_diagnostics_rank()
    e.close()
    e = _engine(64, 5)
    e.set_state(np.random.RandomState(2).normal(size=(64, 5)))
    e.begin_run()
    e.step(20)
    s = _over(e)
    with pytest.raises(L.BpmError, match=r"bpm_rank_history: a window of 7 history rows gives half-chains of 3 draws; at least 4 are needed"):
        s.convergence_diagnostics_rank(n_burn=64 * 14)
    with pytest.raises(L.BpmError, match="at least 4"):
        s.rank_history(n_burn=64 * 14)

    def dest(**kw):
        args = dict(algo=L.ALGO_DEMC, n_chains=64, dim=5, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=0, burnin_gen=0)
        args.update(kw)
        return HipEngine(**args)

    for kw, text in ((dict(dim=6), "bpm_rank_history: the destination has dim 6; the source has 5"),
                     (dict(n_chains=32), "bpm_rank_history: the destination has n_chains 32; the source has 64"),
                     (dict(keep_history=False), "bpm_rank_history: the destination needs keep_history=True")):
        bad = dest(**kw)
        with pytest.raises(L.BpmError, match=text):
            e.rank_history(0, 21, 1, dst=bad)
        bad.close()
    with pytest.raises(L.BpmError, match="bpm_rank_history: the destination is the source itself"):
        e.rank_history(0, 21, 1, dst=e)
    with pytest.raises(L.BpmError, match=r"bpm_rank_history: kind 3 needs arg"):
        e.rank_history(0, 21, 3)
    with pytest.raises(L.BpmError, match=r"bpm_rank_history: order statistic 1280 is outside \[0, 1280\)"):
        e.rank_history(0, 21, 0, None, [1280])
    monkeypatch.setenv("BPM_RANK_SCRATCH_MB", "0")
    with pytest.raises(L.BpmError, match=r"bpm_rank_history: sorting one column of 1280 keys needs \d+ bytes of scratch \(keys in, keys out and the "
                                         r"sort's temporaries\); the budget is 0 bytes"):
        s.convergence_diagnostics_rank()
    monkeypatch.delenv("BPM_RANK_SCRATCH_MB")
    good = dest()
    e.rank_history(0, 21, 0, dst=good)                                 # ... and the same handles, in order, work
    assert good.history_rows() == 20
    good.close()
    with pytest.raises(ValueError, match="rank_history: scale must be 'z' or 'rank'"):
        s.rank_history(scale="u")
    e.close()
    from bipymc_amd.samplers import DeMc
    with pytest.raises(RuntimeError, match="convergence_diagnostics_rank: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).convergence_diagnostics_rank()
