"""Posterior covariance on the GPU (bpm_reduce_cov + bipymc_amd/covariance.py): the lane map of the FP64 matrix instruction on exact
integers first, then every result against np.cov(param_est(n_burn)[2], rowvar=False) -- installed histories with padding, a constant
column, ties, NaN, inf and signed zeros; sampler histories (shuffled DREAM, snooker, wide rows, the serial class); cfg2's size; across
ranks; no side effects; errors.

Tolerance: the derived bound of tests/test_covariance_host.py (its docstring), element by element
    |cov_dev - cov_numpy| <= 2 (n + 4) u sqrt(C_ii C_jj),   |mean_dev - mean_numpy| <= 2 (n + 4) u (|mean| + sqrt(C_kk)),
and (n + 4) u sqrt(C_ii C_jj) against a np.longdouble two-pass covariance where n <= 10^5.  Nothing else."""
import os
import statistics
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from _history_cases import _dream_class, _engine, group_single_rank, local_group, per_rank, run_rank_processes  # noqa: E402
from test_covariance_host import check_against_numpy, cov_bound  # noqa: E402


def _device(eng, n_burn):
    from bipymc_amd import covariance as CV
    return CV.compute(eng.reduce_moments, eng.reduce_cov, CV.single_process_allgather, n_burn, eng.dim)


def _check(pc, rows):
    rows = np.asarray(rows)
    with np.errstate(invalid="ignore"):
        check_against_numpy(pc, rows, long_double=rows.shape[0] <= 10 ** 5)


def _same_bits(a, b):
    assert a.n == b.n
    assert np.array_equal(a.cov.view(np.uint64), b.cov.view(np.uint64))
    assert np.array_equal(a.mean.view(np.uint64), b.mean.view(np.uint64))


@pytest.mark.parametrize("d", [16, 21])
def test_mfma_lane_map_on_exact_integers(d):
    """|x| <= 8, 40 rows: every product and every partial sum is an integer below 2^53, so whatever the order of the sums the device must
    return the integer X^T X exactly -- a wrong lane, row or column map cannot (X^T X's off-diagonal tile of d = 21 is not symmetric)"""
    N, G = 8, 5
    X = np.random.RandomState(11).randint(-8, 9, size=(G, N, d)).astype(np.float64)
    e = _engine(N, d)
    e.set_history(X, X[-1])
    R = X.reshape(-1, d)
    for n_burn in (0, 3, 17):
        cnt, s1, s2 = e.reduce_cov(n_burn, np.zeros(d))
        assert cnt == G * N - n_burn
        assert np.array_equal(s2, R[n_burn:].T @ R[n_burn:])
        assert np.array_equal(s1, R[n_burn:].sum(axis=0))
    c = np.arange(d, dtype=np.float64) - 3.0            # an integer centre: still exact
    cnt, s1, s2 = e.reduce_cov(0, c)
    assert np.array_equal(s2, (R - c).T @ (R - c))
    assert np.array_equal(s1, (R - c).sum(axis=0))
    e.close()


def test_installed_history_with_padding_constant_ties_nan_inf_and_signed_zeros():
    N, d, G = 256, 5, 40                        # d = 5: one padding column per row, eleven more in the tile
    rs = np.random.RandomState(7)
    X = rs.normal(size=(G, N, d))
    X[:, :, 0] = 0.5                            # a constant coordinate
    X[:, :, 1] = np.round(X[:, :, 1] * 3.0)     # many exact ties
    X[8:12, :, 4] = -0.0
    X[12:16, :, 4] = 0.0
    e = _engine(N, d)
    e.set_history(X, X[-1])
    R = X.reshape(-1, d)
    for n_burn in (0, 1, N * 3 + 5, N * 10, G * N - 2):
        pc = _device(e, n_burn)
        _check(pc, R[n_burn:])
        assert pc.mean[0] == 0.5                # the centre of a constant column is the constant ...
        assert np.all(pc.cov[0] == 0.0) and np.all(pc.cov[:, 0] == 0.0)      # ... so its row and column are exactly 0
    c = _device(e, 0).corr()
    assert np.isnan(c[0]).all() and np.isnan(c[:, 0]).all() and np.all(np.diag(c)[1:] == 1.0)
    X[3, 17, 2] = np.nan                        # a NaN column (earlier rows only: the last row is the state)
    X[:5, :, 3] = np.inf
    X[5:8, :100, 3] = -np.inf
    e.set_history(X, X[-1])
    R = X.reshape(-1, d)
    for n_burn in (0, N * 3 + 5, N * 10):       # (from generation 10 on the window holds neither the NaN nor an infinity)
        pc = _device(e, n_burn)
        _check(pc, R[n_burn:])
    assert np.isnan(_device(e, 0).cov[2]).all() and np.isnan(_device(e, 0).cov[:, 3]).all()
    assert not np.isnan(_device(e, N * 10).cov).any()
    # the padding columns hold zeros: a posterior far from zero must never see them
    Y = rs.normal(size=(G, N, d)) + 1e6
    e.set_history(Y, Y[-1])
    _check(_device(e, 0), Y.reshape(-1, d))
    e.close()


def test_installed_history_dim_1800():
    """the widest rows README quotes: 113 column tiles, 29 blocks of 4, 435 block pairs"""
    N, d, G = 8, 1800, 6
    rs = np.random.RandomState(9)
    X = rs.normal(size=(G, N, d)) + np.linspace(-5.0, 5.0, d)
    X[:, :, 1:] += 0.5 * X[:, :, :-1]
    e = _engine(N, d)
    e.set_history(X, X[-1])
    for n_burn in (0, N + 3):
        _check(_device(e, n_burn), X.reshape(-1, d)[n_burn:])
    e.close()


def test_dream_shuffled_history_partial_generation():
    N = 1024
    s = _dream_class(N, 100, 300)
    n_burn = N * 40 + 5
    pc = s.param_est_cov(n_burn)
    _check(pc, s.param_est(n_burn)[2])
    assert pc.cov.shape == (100, 100) and pc.mean.shape == (100,)
    _same_bits(pc, s.param_est_cov(n_burn))
    _check(s.param_est_cov(), s.param_est(0)[2])


def test_demc_banana_with_snooker():
    from bipymc_amd.demc import DeMcMpi
    from bipymc_amd.utils import banana_rv
    s = DeMcMpi(banana_rv.Banana_2D().ln_like, np.zeros(2), n_chains=512, seed=99, p_snooker=0.2)
    s.run_mcmc(512 * 400)
    n_burn = 512 * 100 + 77
    _check(s.param_est_cov(n_burn), s.param_est(n_burn)[2])


def test_wide_rows():
    N = 64
    s = _dream_class(N, 640, 150)
    n_burn = N * 10 + 1
    _check(s.param_est_cov(n_burn), s.param_est(n_burn)[2])


def test_serial_demc():
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.3, dim=6)
    s = DeMc(t.ln_like, n_chains=64, seed=8)
    s.run_mcmc(64 * 300, np.zeros(6))
    n_burn = 64 * 50 + 1
    _check(s.param_est_cov(n_burn), s.param_est(n_burn)[2])


def test_cfg2_size():
    """N = 8192, d = 100, 120 generations (0.8 GB of history)"""
    e = _engine(8192, 100, burnin_gen=100, n_cr_gen=20)
    e.set_state(np.random.RandomState(4).normal(size=(8192, 100)) * np.sqrt(np.arange(100) + 1.0))
    e.begin_run()
    e.step(120)
    n_burn = 8192 * 20 + 100
    got = _device(e, n_burn)
    H = e.get_history()
    e.close()
    _check(got, H.reshape(-1, 100)[n_burn:])


def test_equicorrelated_target_reports_rho():
    """After burn-in the mean off-diagonal correlation must be rho within the Monte-Carlo error the run's own effective sample size implies.
    A sample correlation r of n_eff independent draws of a bivariate normal has the large-sample standard deviation (1 - rho^2) / sqrt(n_eff)
    (Fisher); the mean of the off-diagonal entries varies no more than one of them, and the smallest ESS over coordinates
    (convergence_diagnostics) stands for n_eff.  z is the two-sided normal quantile of a false-alarm probability of 1e-6, computed, so
        |mean offdiag corr - rho| <= z (1 - rho^2) / sqrt(min ESS)."""
    rho, d, N = 0.5, 10, 256
    s = _dream_class(N, d, 2000, rho=rho)
    n_burn = N * 500
    c = s.param_est_cov(n_burn).corr()
    ess = float(np.min(s.convergence_diagnostics(n_burn).ess))
    off = c[~np.eye(d, dtype=bool)]
    z = statistics.NormalDist().inv_cdf(1.0 - 0.5e-6)
    err = abs(float(np.mean(off)) - rho)
    print("mean off-diagonal correlation %.5f, rho %.2f, min ESS %.0f, allowed %.5f" % (float(np.mean(off)), rho, ess, z * (1 - rho ** 2) / np.sqrt(ess)))
    assert err <= z * (1.0 - rho ** 2) / np.sqrt(ess)
    assert np.all(np.diag(c) == 1.0) and np.array_equal(c, c.T)


def test_no_side_effects_and_repeat_call_bit_identical():
    a = _engine(256, 12)
    a.set_state(np.random.RandomState(1).normal(size=(256, 12)))
    a.begin_run()
    a.step(100)
    _same_bits(_device(a, 256 * 3 + 9), _device(a, 256 * 3 + 9))
    a.step(100)
    b = _engine(256, 12)
    b.set_state(np.random.RandomState(1).normal(size=(256, 12)))
    b.begin_run()
    b.step(200)
    assert np.array_equal(a.get_history(), b.get_history())
    assert np.array_equal(a.get_state(), b.get_state())
    assert np.array_equal(a.get_loglike(), b.get_loglike())
    a.close()
    b.close()


def test_errors_say_what_is_wrong():
    from bipymc_amd import _lib as L
    for kw in (dict(keep_history=False), dict(keep_history=False, running_moments=True)):
        e = _engine(64, 4, burnin_gen=0, **kw)
        e.set_state(np.zeros((64, 4)) + np.arange(4))
        e.begin_run()
        e.step(10)
        with pytest.raises(L.BpmError, match="needs keep_history=True"):
            _device(e, 0)
        with pytest.raises(L.BpmError, match="needs keep_history=True"):
            e.reduce_cov(0, np.zeros(4))
        e.close()
    e = _engine(64, 4)
    e.set_state(np.random.RandomState(2).normal(size=(64, 4)))
    e.begin_run()
    e.step(20)
    with pytest.raises(L.BpmError, match="null argument"):
        e.reduce_cov(0, None)
    with pytest.raises(ValueError, match="window is empty"):
        _device(e, 21 * 64)
    with pytest.raises(ValueError, match="window is empty"):
        _device(e, 10 ** 9)
    with pytest.raises(ValueError, match="at least 2 rows"):
        _device(e, 21 * 64 - 1)
    assert _device(e, 21 * 64 - 2).n == 2
    assert e.reduce_cov(64 * 20 + 3, np.zeros(4))[0] == 61
    e.close()


def test_dim_beyond_the_limit_is_named():
    from bipymc_amd import _lib as L
    d = 16400
    e = _engine(4, d)
    X = np.random.RandomState(3).normal(size=(2, 4, d))
    e.set_history(X, X[-1])
    with pytest.raises(L.BpmError, match="beyond the supported limit of 16384"):
        e.reduce_cov(0, np.zeros(d))
    e.close()


def _group_cov(R):
    from bipymc_amd import covariance as CV
    ranks, N, d = local_group(R)
    n_burn = N * 7 + N // 2 + 1                 # a partial generation that starts inside a later rank's chains
    # every rank runs the driver on the gathered parts, as a communicator's allgather hands them out
    res = [CV.compute(per_rank(ranks, "reduce_moments"), per_rank(ranks, "reduce_cov"), lambda x: x, n_burn, d) for _ in ranks]
    for e in ranks:
        e.close()
    one = group_single_rank()
    ref = _device(one, n_burn)
    H = one.get_history()
    one.close()
    return res, ref, H.reshape(-1, d)[n_burn:]


@pytest.mark.parametrize("R", [2, 4])
def test_local_group_against_single_rank(R):
    res, ref, rows = _group_cov(R)
    _check(ref, rows)
    for r in res[1:]:
        _same_bits(r, res[0])
    _check(res[0], rows)
    want = np.cov(rows, rowvar=False)
    assert np.all(np.abs(res[0].cov - ref.cov) <= cov_bound(ref.n, want))


def test_rank_processes_sharing_the_gpu(tmp_path):
    one, r = run_rank_processes(tmp_path, "cov")
    from bipymc_amd.covariance import PosteriorCovariance
    pcs = [PosteriorCovariance(x["mean"], x["cov"], int(x["n"])) for x in [one] + r]
    _check(pcs[0], one["chain_slice"])
    _same_bits(pcs[1], pcs[2])
    _check(pcs[1], one["chain_slice"])
    want = np.cov(one["chain_slice"], rowvar=False)
    assert np.all(np.abs(pcs[1].cov - pcs[0].cov) <= cov_bound(pcs[0].n, want))
