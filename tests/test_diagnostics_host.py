"""Convergence diagnostics, host side (no GPU): bipymc_amd/diagnostics.py's finishing layer against an independent NumPy restatement of
split-chain R-hat and ESS, Geyer's truncation on hand-built sequences, and the collective over a gloo world of 2 ranks."""
import os
import socket

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- independent restatement (full (G, N, d) history) --------------------------------------------------------------------------------
def ref_geyer(rho, n, m, max_lag=None):
    """rho: autocorrelations at lags 0 ... n - 1.  Stan / ArviZ ess(method="mean"), with an optional lag cap -> (tau, capped, max_t)"""
    rho_hat_t = np.zeros(n)
    rho_hat_even = 1.0
    rho_hat_t[0] = rho_hat_even
    rho_hat_odd = rho[1]
    rho_hat_t[1] = rho_hat_odd
    capped = False
    t = 1
    while t < (n - 3) and (rho_hat_even + rho_hat_odd) > 0.0:
        if max_lag is not None and t + 2 > max_lag:
            capped = True
            break
        rho_hat_even = rho[t + 1]
        rho_hat_odd = rho[t + 2]
        if (rho_hat_even + rho_hat_odd) >= 0:
            rho_hat_t[t + 1] = rho_hat_even
            rho_hat_t[t + 2] = rho_hat_odd
        t += 2
    max_t = t - 2
    if rho_hat_even > 0:
        rho_hat_t[max_t + 1] = rho_hat_even
    t = 1
    while t <= max_t - 2:
        if (rho_hat_t[t + 1] + rho_hat_t[t + 2]) > (rho_hat_t[t - 1] + rho_hat_t[t]):
            rho_hat_t[t + 1] = (rho_hat_t[t - 1] + rho_hat_t[t]) / 2.0
            rho_hat_t[t + 2] = rho_hat_t[t + 1]
        t += 2
    tau = -1.0 + 2.0 * np.sum(rho_hat_t[:max_t + 1]) + np.sum(rho_hat_t[max_t + 1:max_t + 2])
    tau = max(tau, 1.0 / np.log10(m * n))
    return tau, capped, max_t


def reference(X, g0=0, max_lag=None):
    """X: (G_rows, N, d) history.  -> dict r_hat, ess, tau, capped, margin (|sum of the pair that ended the sequence|), rho"""
    X = np.asarray(X, dtype=np.float64)[g0:]
    G = X.shape[0]
    n = G // 2
    halves = np.concatenate([X[:n], X[G - n:]], axis=1)            # (n, 2N, d): half-chains side by side
    m = halves.shape[1]
    xbar = halves.mean(axis=0)
    s2 = halves.var(axis=0, ddof=1)
    W = s2.mean(axis=0)
    Bn = xbar.var(axis=0, ddof=1)
    varp = (n - 1.0) / n * W + Bn
    with np.errstate(divide="ignore", invalid="ignore"):
        r_hat = np.sqrt(varp / W)
    # biased autocovariance of every half-chain by FFT, coordinate by coordinate
    d = X.shape[2]
    C = np.empty((n, d))
    for k in range(d):
        y = halves[:, :, k] - xbar[:, k]
        f = np.fft.rfft(y, n=2 * n, axis=0)
        C[:, k] = (np.fft.irfft(f * np.conj(f), n=2 * n, axis=0)[:n] / n).mean(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = 1.0 - (W - C) / varp
    tau = np.full(d, np.nan)
    capped = np.zeros(d, dtype=bool)
    margin = np.full(d, np.inf)
    for k in range(d):
        if not W[k] > 0:
            r_hat[k] = np.nan
            continue
        tau[k], capped[k], max_t = ref_geyer(rho[:, k], n, m, max_lag)
        if not capped[k] and max_t + 3 < n:
            margin[k] = abs(rho[max_t + 1, k] + rho[max_t + 2, k])
    return dict(r_hat=r_hat, ess=m * n / tau, tau=tau, capped=capped, margin=margin, rho=rho, n=n, m=m)


# ---- NumPy stand-ins for the two device reductions, on one block of chains ---------------------------------------------------------------
class BlockParts(object):
    """what bpm_diag_split_moments / bpm_diag_autocov return for the chains of one rank: H = (rows, n_local, d)"""

    def __init__(self, H):
        self.H = np.asarray(H, dtype=np.float64)
        self.win = None

    def split(self, g0, g1):
        n = (g1 - g0) // 2
        if n < 4:
            raise RuntimeError("bpm_diag_split_moments: at least 4 draws per half-chain are needed")
        h = np.concatenate([self.H[g0:g0 + n], self.H[g1 - n:g1]], axis=1)
        xbar = h.mean(axis=0)
        mu = xbar.mean(axis=0)
        self.win = (h, xbar, n)
        return mu, ((xbar - mu) ** 2).sum(axis=0), h.var(axis=0, ddof=1).sum(axis=0), h.shape[1], n

    def autocov(self, t0, n_lags):
        if self.win is None:
            raise RuntimeError("bpm_diag_autocov: call bpm_diag_split_moments first")
        h, xbar, n = self.win
        assert t0 + n_lags <= n
        y = h - xbar
        return np.stack([(y[:n - t] * y[t:]).sum(axis=0).sum(axis=0) / n for t in range(t0, t0 + n_lags)])


def _diag_from_blocks(H, n_blocks, g0=0, max_lag=None):
    from bipymc_amd import diagnostics as D
    blocks = [BlockParts(b) for b in np.array_split(H, n_blocks, axis=1)]
    return D.compute(lambda a, b: [p.split(a, b) for p in blocks],
                     lambda t0, nl: [p.autocov(t0, nl) for p in blocks],
                     lambda x: x, g0, H.shape[0], max_lag=max_lag)


def _ar1(G, N, phis, seed, offset=None):
    rs = np.random.RandomState(seed)
    phis = np.asarray(phis, dtype=np.float64)
    X = np.empty((G, N, len(phis)))
    X[0] = rs.normal(size=(N, len(phis))) / np.sqrt(1 - phis ** 2)
    for g in range(1, G):
        X[g] = phis * X[g - 1] + rs.normal(size=(N, len(phis)))
    if offset is not None:
        X += offset
    return X


@pytest.mark.parametrize("n_blocks", [1, 2, 4])
@pytest.mark.parametrize("G", [201, 120])
def test_finishing_layer_equals_numpy_restatement(n_blocks, G):
    X = _ar1(G, 16, [0.0, 0.5, 0.9, 0.3, -0.2], seed=3)
    X[:, :8, 3] += 1.5                                 # between-chain disagreement on one coordinate
    ref = reference(X)
    got = _diag_from_blocks(X, n_blocks)
    assert got.n_half_chains == ref["m"] == 32 and got.n_draws == ref["n"] == G // 2
    np.testing.assert_allclose(got.r_hat, ref["r_hat"], rtol=1e-13)
    np.testing.assert_allclose(got.tau, ref["tau"], rtol=1e-13)
    np.testing.assert_allclose(got.ess, ref["ess"], rtol=1e-13)
    assert not got.ess_capped.any()
    assert got.window == (0, G)
    assert got.r_hat[3] > 1.1


def test_window_starts_at_the_first_whole_generation():
    from bipymc_amd import diagnostics as D
    assert D.window(0, 8, 50) == (0, 50)
    assert D.window(8, 8, 50) == (1, 50)
    assert D.window(9, 8, 50) == (2, 50)
    X = _ar1(90, 8, [0.5, 0.7], seed=5)
    got = _diag_from_blocks(X, 2, g0=D.window(17, 8, 90)[0])
    ref = reference(X, g0=3)
    np.testing.assert_allclose(got.ess, ref["ess"], rtol=1e-13)
    assert got.window == (3, 90) and got.n_draws == 43


def test_max_lag_caps_the_sum_and_says_so():
    X = _ar1(401, 8, [0.95, 0.0], seed=7)
    ref = reference(X, max_lag=6)
    got = _diag_from_blocks(X, 2, max_lag=6)
    assert got.ess_capped[0] and ref["capped"][0]
    assert not got.ess_capped[1]
    np.testing.assert_allclose(got.tau, ref["tau"], rtol=1e-13)
    assert got.lags_used[0] <= 7
    full = _diag_from_blocks(X, 2)
    assert not full.ess_capped.any() and full.lags_used[0] > 7


def test_geyer_on_hand_built_sequences():
    from bipymc_amd.diagnostics import geyer
    n, m = 100, 4

    def ref(rho):
        return ref_geyer(np.r_[rho, np.zeros(n - len(rho))], n, m)[0]

    # early stop: the pair (rho_4, rho_5) sums below zero -> max_t = 3; its even value (> 0) is kept as rho_4
    rho = np.array([1.0, 0.5, 0.2, 0.1, 0.3, -0.5, 0.9, 0.9])
    tau, lags, capped = geyer(rho, n, m, n - 1)
    assert (lags, capped) == (6, False)
    assert tau == ref(rho) and tau == pytest.approx(-1.0 + 2.0 * (1.0 + 0.5 + 0.2 + 0.1) + 0.3, rel=1e-15)
    # ... and without the kept value when it is negative
    rho = np.array([1.0, 0.5, 0.2, 0.1, -0.3, -0.1, 0.9, 0.9])
    tau, lags, capped = geyer(rho, n, m, n - 1)
    assert tau == ref(rho) and tau == pytest.approx(-1.0 + 2.0 * 1.8, rel=1e-15)
    # monotone repair: pair (rho_2, rho_3) sums higher than (rho_0, rho_1) -> both become the average of the earlier pair
    rho = np.array([1.0, -0.5, 0.6, 0.3, 0.1, -0.3, 0.0, 0.0])
    tau, lags, capped = geyer(rho, n, m, n - 1)
    assert tau == ref(rho) and tau == pytest.approx(-1.0 + 2.0 * (1.0 - 0.5 + 0.25 + 0.25) + 0.1, rel=1e-15)
    # the first pair already non-positive: tau is clamped to 1 / log10(m n)
    tau, lags, capped = geyer(np.array([1.0, -1.2, 0.1, 0.1]), n, m, n - 1)
    assert tau == 1.0 / np.log10(m * n) and lags == 2
    # more lags needed -> None; the cap -> capped
    assert geyer(np.array([1.0, 0.9, 0.8, 0.7]), n, m, n - 1) is None
    tau, lags, capped = geyer(np.array([1.0, 0.9, 0.8, 0.7]), n, m, 3)
    assert capped and lags == 4 and tau == pytest.approx(-1.0 + 2.0 * 1.9 + 0.8, rel=1e-15)
    assert tau == ref_geyer(np.r_[[1.0, 0.9, 0.8, 0.7], np.zeros(n - 4)], n, m, max_lag=3)[0]


def test_constant_coordinate_is_nan():
    X = _ar1(60, 8, [0.5, 0.5, 0.5], seed=2)
    X[:, :, 1] = 2.5
    got = _diag_from_blocks(X, 2)
    assert np.isnan(got.r_hat[1]) and np.isnan(got.ess[1]) and np.isnan(got.tau[1])
    assert np.isfinite(got.r_hat[[0, 2]]).all() and np.isfinite(got.ess[[0, 2]]).all()


def test_too_short_window_is_an_error():
    with pytest.raises(RuntimeError, match="at least 4"):
        _diag_from_blocks(_ar1(7, 8, [0.5], seed=1), 1)


# ---- the collective over torch.distributed / gloo ------------------------------------------------------------------------------------------
def _engine_factory(**kw):
    import sys
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    from _oracle_engine import OracleEngine

    class DiagOracleEngine(OracleEngine):
        """the oracle engine plus the two diagnostic reductions in NumPy (what the HIP engine does on the device)"""

        def diag_split_moments(self, g_lo, g_hi):
            self._diag = BlockParts(np.stack(self.s.history, axis=0))
            mu, m2, sv, m, n = self._diag.split(g_lo, g_hi)
            return mu, m2, sv, m, n

        def diag_autocov(self, t0, n_lags):
            return self._diag.autocov(t0, n_lags)

    return DiagOracleEngine(**kw)


def _run_dream(comm):
    from bipymc_amd.dream import DreamMpi
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.5, dim=5)
    s = DreamMpi(t.ln_like, np.zeros(5), n_chains=12, mpi_comm=comm, n_cr_gen=3, burnin_gen=8, seed=4321)
    s.run_mcmc(12 * 40)
    return s.convergence_diagnostics(n_burn=12 * 5 + 7), s.convergence_diagnostics(max_lag=5)


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    import bipymc_amd.demc as _demc
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        _demc._engine_factory = _engine_factory
        a, b = _run_dream("torch")
        np.savez(os.path.join(out_dir, "diag_rank%d.npz" % rank), **{"a_" + f: np.asarray(getattr(a, f)) for f in a._fields},
                 **{"b_" + f: np.asarray(getattr(b, f)) for f in b._fields})
    finally:
        dist.barrier()
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_gloo_ranks_agree_bitwise_and_equal_one_rank(tmp_path, monkeypatch):
    import torch.multiprocessing as mp
    import bipymc_amd.demc as _demc
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [np.load(os.path.join(str(tmp_path), "diag_rank%d.npz" % k)) for k in range(2)]
    for f in r[0].files:
        assert np.array_equal(r[0][f], r[1][f], equal_nan=True), f          # the same bits on every rank
    monkeypatch.setattr(_demc, "_engine_factory", _engine_factory)
    a, b = _run_dream(None)
    for pre, one in (("a_", a), ("b_", b)):
        np.testing.assert_allclose(r[0][pre + "r_hat"], one.r_hat, rtol=1e-12)
        np.testing.assert_allclose(r[0][pre + "ess"], one.ess, rtol=1e-12)
        assert np.array_equal(r[0][pre + "ess_capped"], one.ess_capped)
        assert np.array_equal(r[0][pre + "lags_used"], one.lags_used)
        assert int(r[0][pre + "n_half_chains"]) == one.n_half_chains == 24
    assert tuple(a.window) == (6, 40) and b.ess_capped.any()
