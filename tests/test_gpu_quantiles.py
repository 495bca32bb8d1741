"""Posterior quantiles on the GPU (bpm_quantile_begin / bpm_quantile_histogram + bipymc_amd/quantiles.py): every result must equal
np.quantile(param_est(n_burn)[2], q, axis=0) value for value (np.array_equal, equal_nan=True) -- on installed histories with NaN, inf,
signed zeros, ties and padding columns, on sampler histories (shuffled DREAM, snooker, wide rows, the serial class), at cfg2's size,
across ranks; no side effects; errors."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from _history_cases import _dream_class, _engine, group_single_rank, local_group, per_rank, run_rank_processes  # noqa: E402

QS = [0.0, 0.05, 0.5, 1.0 / 3.0, 0.95, 1.0]


def _device(eng, n_burn, q=QS):
    from bipymc_amd import quantiles as Q
    return Q.compute(eng.quantile_begin, eng.quantile_histogram, Q.single_process_allgather, n_burn, q, dim=eng.dim)


def _want(H, n_burn, q=QS):
    H = np.asarray(H)
    return np.quantile(H.reshape(-1, H.shape[-1])[n_burn:], q, axis=0)


def _same(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))


def test_installed_history_with_nan_inf_signed_zeros_and_ties():
    N, d, G = 256, 5, 40                        # d = 5: one padding column per row
    rs = np.random.RandomState(7)
    X = rs.normal(size=(G, N, d))
    X[:, :, 0] = 0.5                            # a constant coordinate
    X[:, :, 1] = np.round(X[:, :, 1] * 3.0)     # many exact ties
    X[3, 17, 2] = np.nan                        # a NaN column (earlier rows only: the last row is the state)
    X[:5, :, 3] = np.inf
    X[5:8, :100, 3] = -np.inf
    X[8:12, :, 4] = -0.0
    X[12:16, :, 4] = 0.0
    e = _engine(N, d)
    e.set_history(X, X[-1])
    for n_burn in (0, 1, N * 3 + 5, N * 10, G * N - 1):
        _same(_device(e, n_burn), _want(X, n_burn))
    _same(_device(e, 0, [0.5, 1.0]), _want(X, 0, [0.5, 1.0]))
    # the padding column holds zeros: a coordinate entirely below zero must never see them
    Y = -np.abs(rs.normal(size=(G, N, d))) - 1.0
    e.set_history(Y, Y[-1])
    got = _device(e, 0, [0.0, 1.0])
    assert (got < 0).all()
    _same(got, _want(Y, 0, [0.0, 1.0]))
    e.close()


def test_dream_shuffled_history_partial_generation():
    N = 1024
    s = _dream_class(N, 100, 300)
    n_burn = N * 40 + 5
    chain_slice = s.param_est(n_burn)[2]
    _same(s.param_est_quantiles(n_burn, QS), np.quantile(chain_slice, QS, axis=0))
    _same(s.param_est_quantiles(n_burn), np.quantile(chain_slice, (0.05, 0.5, 0.95), axis=0))
    _same(s.param_est_quantiles(n_burn, 0.5), np.quantile(chain_slice, 0.5, axis=0))
    _same(s.param_est_quantiles(n_burn, 0), np.quantile(chain_slice, 0, axis=0))
    _same(s.param_est_quantiles(n_burn, [0, 1]), np.quantile(chain_slice, [0, 1], axis=0))
    assert s.param_est_quantiles(n_burn, 0.5).shape == (100,)


def test_demc_banana_with_snooker():
    from bipymc_amd.demc import DeMcMpi
    from bipymc_amd.utils import banana_rv
    s = DeMcMpi(banana_rv.Banana_2D().ln_like, np.zeros(2), n_chains=512, seed=99, p_snooker=0.2)
    s.run_mcmc(512 * 400)
    n_burn = 512 * 100 + 77
    _same(s.param_est_quantiles(n_burn, QS), np.quantile(s.param_est(n_burn)[2], QS, axis=0))


def test_wide_rows():
    N = 64
    s = _dream_class(N, 640, 150)
    n_burn = N * 10 + 1
    _same(s.param_est_quantiles(n_burn, QS), np.quantile(s.param_est(n_burn)[2], QS, axis=0))


def test_serial_demc():
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.3, dim=6)
    s = DeMc(t.ln_like, n_chains=64, seed=8)
    s.run_mcmc(64 * 300, np.zeros(6))
    n_burn = 64 * 50 + 1
    _same(s.param_est_quantiles(n_burn, QS), np.quantile(s.param_est(n_burn)[2], QS, axis=0))
    _same(s.param_est_quantiles(n_burn, 0.95), np.quantile(s.param_est(n_burn)[2], 0.95, axis=0))


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
    _same(got, _want(H, n_burn))


def test_no_side_effects():
    a = _engine(256, 12)
    a.set_state(np.random.RandomState(1).normal(size=(256, 12)))
    a.begin_run()
    a.step(100)
    r1 = _device(a, 256 * 3 + 9)
    r2 = _device(a, 256 * 3 + 9)
    assert np.array_equal(r1.view(np.uint64), r2.view(np.uint64))
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
        e.close()
    e = _engine(64, 4)
    e.set_state(np.random.RandomState(2).normal(size=(64, 4)))
    e.begin_run()
    with pytest.raises(L.BpmError, match="call bpm_quantile_begin first"):
        e.quantile_histogram([0], [0], 0)
    e.step(20)
    with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
        _device(e, 0, [0.5, 1.5])
    with pytest.raises(ValueError, match="window is empty"):
        _device(e, 21 * 64)
    with pytest.raises(ValueError, match="window is empty"):
        _device(e, 10 ** 9)
    assert e.quantile_begin(64 * 20 + 3) == 61
    e.quantile_histogram([0, 1], [0, 0], 0)
    with pytest.raises(L.BpmError, match="sorted by coordinate"):
        e.quantile_histogram([1, 0], [0, 0], 0)
    with pytest.raises(L.BpmError, match="coordinate out of range"):
        e.quantile_histogram([4], [0], 0)
    with pytest.raises(L.BpmError, match="prefix_bits"):
        e.quantile_histogram([0], [0], 4)
    e.step(1)
    with pytest.raises(L.BpmError, match="history changed"):
        e.quantile_histogram([0], [0], 0)
    e.quantile_begin(0)
    e.set_state(np.zeros((64, 4)))
    with pytest.raises(L.BpmError, match="history changed"):
        e.quantile_histogram([0], [0], 0)
    e.close()


def _group_quantiles(R):
    from bipymc_amd import quantiles as Q
    ranks, N, d = local_group(R)
    n_burn = N * 7 + N // 2 + 1                 # a partial generation that starts inside a later rank's chains
    res = Q.compute(per_rank(ranks, "quantile_begin"), per_rank(ranks, "quantile_histogram"), lambda x: x, n_burn, QS, dim=d)
    for e in ranks:
        e.close()
    one = group_single_rank()
    ref = _device(one, n_burn)
    H = one.get_history()
    one.close()
    return res, ref, _want(H, n_burn)


@pytest.mark.parametrize("R", [2, 4])
def test_local_group_equals_single_rank(R):
    res, ref, want = _group_quantiles(R)
    _same(ref, want)
    assert np.array_equal(res.view(np.uint64), ref.view(np.uint64))


def test_rank_processes_sharing_the_gpu(tmp_path):
    one, r = run_rank_processes(tmp_path, "quantiles")
    from _stats_worker import Q
    _same(one["q"], np.quantile(one["chain_slice"], Q, axis=0))
    assert np.array_equal(r[0]["q"].view(np.uint64), r[1]["q"].view(np.uint64))
    _same(r[0]["q"], one["q"])
