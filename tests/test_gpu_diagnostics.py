"""Convergence diagnostics on the GPU (bpm_diag_split_moments / bpm_diag_autocov + bipymc_amd/diagnostics.py): split-chain R-hat and ESS
of the resident history against the NumPy restatement of tests/test_diagnostics_host.py, on installed AR(1) histories with known answers,
on sampler histories (position-ordered, snooker, wide rows, the serial class), at cfg2's size, across ranks; no side effects; errors.

These are large, well-conditioned, finite histories compared on the finished r_hat / ess.  What the two entry points return, at the sizes
where the kernels' tiling changes, on badly conditioned columns and with non-finite values, is held to an exactly rounded reference in
tests/test_gpu_diagnostics_edges.py (tests/_diag_exact.py, tests/test_diag_exact_host.py); that a non-finite value stays in its own
coordinate, for every statistic of the history, in tests/test_gpu_statistics_isolation.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from _history_cases import _dream_class, _engine, group_single_rank, local_group, per_rank, run_rank_processes  # noqa: E402
from test_diagnostics_host import _ar1, reference  # noqa: E402


def _device(eng, g0=0, g1=None, max_lag=None):
    from bipymc_amd import diagnostics as D
    g1 = eng.history_rows() if g1 is None else g1
    return D.compute(eng.diag_split_moments, eng.diag_autocov, D.single_process_allgather, g0, g1, max_lag=max_lag)


def _check(got, ref, rtol_r=1e-10, rtol_e=1e-8):
    np.testing.assert_allclose(got.r_hat, ref["r_hat"], rtol=rtol_r)
    ok = ref["margin"] > 1e-6                   # (a pair sum within rounding of zero could truncate either way)
    assert ok.sum() >= 0.8 * len(ok)
    np.testing.assert_allclose(got.ess[ok], ref["ess"][ok], rtol=rtol_e)
    assert np.array_equal(got.ess_capped, ref["capped"])


PHIS = [0.0, 0.5, 0.9, 0.5, 0.0]


def test_known_answers_on_installed_ar1_histories():
    N, G = 256, 2001                           # d = 5: ld padding; G odd: the middle row is dropped
    X = _ar1(G, N, PHIS, seed=11)
    e = _engine(N, 5)
    e.set_history(X, X[-1])
    got = _device(e)
    ref = reference(X)
    assert got.n_half_chains == 2 * N and got.n_draws == 1000 and got.window == (0, G)
    _check(got, ref)
    rel = got.ess / (got.n_half_chains * got.n_draws)
    want = (1 - np.array(PHIS)) / (1 + np.array(PHIS))
    np.testing.assert_allclose(rel, want, rtol=0.10)
    assert (got.r_hat < 1.01).all()
    # half the chains offset by +1 sigma
    Y = X.copy()
    Y[:, :N // 2, :] += 1.0 / np.sqrt(1.0 - np.array(PHIS) ** 2)
    e.set_history(Y, Y[-1])
    got = _device(e)
    _check(got, reference(Y))
    # the half-chain means split into two groups 1 sigma apart: B/n -> sigma^2 / 4, r_hat -> sqrt(1 + 1/4) = 1.118
    np.testing.assert_allclose(got.r_hat, np.sqrt(1.25), rtol=0.02)
    assert (got.r_hat > 1.1).all()
    # a constant coordinate
    Z = X.copy()
    Z[:, :, 2] = 0.25
    e.set_history(Z, Z[-1])
    got = _device(e)
    assert np.isnan(got.r_hat[2]) and np.isnan(got.ess[2])
    _check(got, reference(Z))
    e.close()


def test_dream_position_ordered_history_against_numpy():
    """DREAM 100-D N=1024, shuffle=True: one GPU appends rows in shuffle order (normalised before the pass); n_burn not a multiple of N"""
    N = 1024
    s = _dream_class(N, 100, 300)
    n_burn = N * 40 + 5
    got = s.convergence_diagnostics(n_burn=n_burn)
    assert got.window == (41, 301)
    H = s._engine.get_history()
    _check(got, reference(H, g0=41))


def test_demc_banana_with_snooker_against_numpy():
    from bipymc_amd.demc import DeMcMpi
    from bipymc_amd.utils import banana_rv
    s = DeMcMpi(banana_rv.Banana_2D().ln_like, np.zeros(2), n_chains=512, seed=99, p_snooker=0.2)
    s.run_mcmc(512 * 400)
    got = s.convergence_diagnostics(n_burn=512 * 100)
    _check(got, reference(s._engine.get_history(), g0=100))


def test_wide_rows_against_numpy():
    N = 64
    s = _dream_class(N, 640, 150)
    got = s.convergence_diagnostics(n_burn=N * 10)
    _check(got, reference(s._engine.get_history(), g0=10))


def test_serial_demc_against_numpy():
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.3, dim=6)
    s = DeMc(t.ln_like, n_chains=64, seed=8)
    s.run_mcmc(64 * 300, np.zeros(6))
    got = s.convergence_diagnostics(n_burn=64 * 50 + 1)
    _check(got, reference(s._engine.get_history(), g0=51))


def test_cfg2_size_against_numpy():
    """N = 8192, d = 100, 400 generations (2.6 GB of history), max_lag = 64"""
    e = _engine(8192, 100, burnin_gen=100, n_cr_gen=20)
    e.set_state(np.random.RandomState(4).normal(size=(8192, 100)) * np.sqrt(np.arange(100) + 1.0))
    e.begin_run()
    e.step(400)
    got = _device(e, max_lag=64)
    H = e.get_history()
    e.close()
    ref = reference(H, max_lag=64)
    _check(got, ref)
    assert got.n_half_chains == 16384 and got.n_draws == 200


def test_no_side_effects():
    a = _engine(256, 12)
    a.set_state(np.random.RandomState(1).normal(size=(256, 12)))
    a.begin_run()
    a.step(100)
    r1 = _device(a, g0=3)
    r2 = _device(a, g0=3)
    for f in ("r_hat", "ess", "tau", "lags_used"):
        assert np.array_equal(getattr(r1, f), getattr(r2, f), equal_nan=True), f
    a.step(100)
    b = _engine(256, 12)
    b.set_state(np.random.RandomState(1).normal(size=(256, 12)))
    b.begin_run()
    b.step(200)
    assert np.array_equal(a.get_history(), b.get_history())
    assert np.array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()


def test_errors_say_what_is_wrong():
    from bipymc_amd import _lib as L
    e = _engine(64, 4, keep_history=False, burnin_gen=0)
    e.set_state(np.zeros((64, 4)) + np.arange(4))
    e.begin_run()
    e.step(10)
    with pytest.raises(L.BpmError, match="needs keep_history=True"):
        e.diag_split_moments(0, 11)
    e.close()
    e = _engine(64, 4, keep_history=False, running_moments=True, burnin_gen=0)
    e.set_state(np.zeros((64, 4)) + np.arange(4))
    e.begin_run()
    e.step(10)
    with pytest.raises(L.BpmError, match="needs keep_history=True"):
        e.diag_split_moments(0, 11)
    e.close()
    e = _engine(64, 4)
    e.set_state(np.random.RandomState(2).normal(size=(64, 4)))
    e.begin_run()
    with pytest.raises(L.BpmError, match="call bpm_diag_split_moments first"):
        e.diag_autocov(0, 4)
    e.step(20)
    with pytest.raises(L.BpmError, match="at least 4"):
        e.diag_split_moments(14, 21)
    e.diag_split_moments(0, 21)
    e.diag_autocov(0, 10)
    with pytest.raises(L.BpmError, match=r"must lie in \[0, n\)"):
        e.diag_autocov(5, 6)
    e.step(1)
    with pytest.raises(L.BpmError, match="history changed"):
        e.diag_autocov(0, 4)
    e.diag_split_moments(0, 22)
    e.set_state(np.zeros((64, 4)))
    with pytest.raises(L.BpmError, match="history changed"):
        e.diag_autocov(0, 4)
    e.close()


def _group_diag(R):
    from bipymc_amd import diagnostics as D
    ranks, N, d = local_group(R)
    g0, g1 = D.window(N * 7 + 1, N, ranks[0].history_rows())
    res = D.compute(per_rank(ranks, "diag_split_moments"), per_rank(ranks, "diag_autocov"), lambda x: x, g0, g1)
    for e in ranks:
        e.close()
    one = group_single_rank()
    ref = _device(one, g0, g1)
    one.close()
    return res, ref


@pytest.mark.parametrize("R", [2, 4])
def test_local_group_equals_single_rank(R):
    res, ref = _group_diag(R)
    np.testing.assert_allclose(res.r_hat, ref.r_hat, rtol=1e-12)
    np.testing.assert_allclose(res.ess, ref.ess, rtol=1e-12)
    assert np.array_equal(res.lags_used, ref.lags_used) and res.n_half_chains == ref.n_half_chains


def test_rank_processes_sharing_the_gpu(tmp_path):
    one, r = run_rank_processes(tmp_path, "diag")
    for f in r[0].files:
        assert np.array_equal(r[0][f], r[1][f], equal_nan=True), f
    np.testing.assert_allclose(r[0]["r_hat"], one["r_hat"], rtol=1e-12)
    np.testing.assert_allclose(r[0]["ess"], one["ess"], rtol=1e-12)
    assert np.array_equal(r[0]["lags_used"], one["lags_used"]) and tuple(r[0]["window"]) == (11, 60)


@pytest.mark.slow
def test_cfg2_from_the_reference_start():
    """cfg2 (8192 chains, 100-D Gaussian) from theta_0 = 0, varepsilon = 1e-6: split-R-hat flags the first 20 generations (observed 1.45) and
    has come down over generations 2000-4000 (observed 1.26: each chain's autocorrelation time is several hundred generations, so half-chains
    of 1000 draws are far from R-hat < 1.01 although the population moments pass their gate from generation 2250 on,
    profiles/r04_convergence_from_reference_start.txt)."""
    e = _engine(8192, 100, burnin_gen=200, n_cr_gen=50)
    e.init_chains(np.zeros(100), np.full(100, 1e-6))
    e.begin_run()
    e.reserve_history(4001)
    e.step(20)
    early = float(np.nanmax(_device(e, 0, 21).r_hat))
    e.step(3980)
    late = _device(e, 2000, 4001)
    e.close()
    print("cfg2 from the reference start: max R-hat gens 0-20 %.4f, gens 2000-4000 %.5f; ESS min / median %.0f / %.0f, tau median %.1f, "
          "lags used max %d" % (early, float(np.nanmax(late.r_hat)), float(np.nanmin(late.ess)), float(np.nanmedian(late.ess)),
                                float(np.nanmedian(late.tau)), int(late.lags_used.max())))
    assert early > 1.1
    assert float(np.nanmax(late.r_hat)) < early
    assert not late.ess_capped.any() and np.isfinite(late.ess).all()
