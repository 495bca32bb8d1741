"""Posterior histograms on the GPU (bpm_hist_range / bpm_hist_marginals / bpm_hist_pairs + bipymc_amd/histograms.py): every count must equal
np.histogram / np.histogram2d on param_est(n_burn)[2] exactly (np.array_equal, no tolerance), every edge np.histogram_bin_edges bit for
bit -- on installed histories with values on and one ulp beside every edge, a large offset with a tiny spread, denormals, a constant
column, NaN and infinities, on sampler histories (DREAM, DE-MC with snooker, the serial class, wide rows), at cfg2's size, across ranks;
no side effects; errors."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from _history_cases import _dream_class, _engine, group_single_rank, local_group, per_rank, run_rank_processes  # noqa: E402
from test_histograms_host import check_against_numpy  # noqa: E402


def _device(eng, n_burn, **kw):
    from bipymc_amd import histograms as HS
    return HS.compute(eng.hist_range, eng.hist_marginals, eng.hist_pairs, HS.single_process_allgather, n_burn, eng.dim, **kw)


def _window(H, n_burn):
    H = np.asarray(H)
    return H.reshape(-1, H.shape[-1])[n_burn:]


def _check(ph, W, kw):
    check_against_numpy(ph, W, kw.get("bins", 20), kw.get("range"), kw.get("bins2d"))


def _invariant(ph):
    """range=None and bins2d == bins: the 2-D counts of a pair sum to the 1-D counts of its members; every 1-D row sums to n"""
    assert np.all(ph.counts.sum(axis=1) == ph.n)
    pos = {int(k): j for j, k in enumerate(ph.dims)}
    for p, (a, b) in enumerate(ph.pairs):
        assert np.array_equal(ph.counts2d[p].sum(axis=1), ph.counts[pos[int(a)]])
        assert np.array_equal(ph.counts2d[p].sum(axis=0), ph.counts[pos[int(b)]])


def _same_bits(a, b):
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)


def _installed(N=256, d=7, G=40):
    """d = 7: one padding column per row.  The last generation (the state) stays finite."""
    rs = np.random.RandomState(7)
    X = rs.normal(size=(G, N, d))
    c0 = rs.uniform(-2.0, 3.0, size=G * N)
    e = np.linspace(-2.0, 3.0, 21)
    plant = np.concatenate([e, np.nextafter(e[1:-1], np.inf), np.nextafter(e[1:-1], -np.inf), np.linspace(-2.0, 3.0, 1025)])
    c0[rs.choice(G * N - N, size=len(plant), replace=False)] = plant     # exactly on every edge, the last included; one ulp either side
    X[:, :, 0] = c0.reshape(G, N)
    X[:, :, 1] = 1e3 + 1e-3 * X[:, :, 1]                                 # a large offset, a tiny spread
    X[:, :, 2] = rs.randint(0, 100, size=(G, N)) * (1024 * 5e-324)      # denormals (1024 bins over them: 99 denormal steps each)
    X[:, :, 3] = 0.7                                                     # constant
    X[3, 17, 4] = np.nan
    X[5, :40, 4] = np.inf
    X[6, 100:130, 4] = -np.inf
    X[:, :, 5] = 0.01 * X[:, :, 5] ** 3                                  # peaked
    return X


@pytest.mark.parametrize("bins,bins2d", [(1, 1), (20, 20), (1024, 64), (20, 64), (7, 1)])
def test_installed_history_edge_values_denormals_constant_column(bins, bins2d):
    X = _installed()
    G, N, d = X.shape
    e = _engine(N, d)
    e.set_history(X, X[-1])
    finite = [0, 1, 2, 3, 5, 6]
    for n_burn in (0, N * 3 + 5, G * N - 1):
        kw = dict(bins=bins, bins2d=bins2d, dims=finite, pairs=[(0, 1), (2, 0), (3, 5), (6, 5), (1, 2), (5, 0)])
        ph = _device(e, n_burn, **kw)
        _check(ph, _window(X, n_burn), kw)
        if bins == bins2d:
            _invariant(ph)
    assert _device(e, 0, dims=[3]).edges[0, 0] == 0.7 - 0.5
    e.close()


@pytest.mark.parametrize("bins,bins2d", [(20, 20), (1024, 64), (1, 1)])
def test_installed_history_explicit_ranges_nan_and_inf(bins, bins2d):
    X = _installed()
    G, N, d = X.shape
    e = _engine(N, d)
    e.set_history(X, X[-1])
    per_dim = [(-2.0, 3.0), (999.999, 1000.0005), (0.0, 5e-324 * 2 ** 14), (0.7, 0.7), (-0.5, 0.5), (-1e-3, 1e-3), (0.25, 0.25)]
    for n_burn in (0, N * 3 + 5):
        W = _window(X, n_burn)
        W2 = np.where(np.isnan(W), 1e300, W)              # (for np.histogram2d: outside the range = counted nowhere)
        for rng in ((-1.0, 1.5), per_dim):
            kw = dict(bins=bins, bins2d=bins2d, range=rng, pairs=[(4, 0), (0, 4), (4, 6), (1, 2), (3, 4)])
            ph = _device(e, n_burn, **kw)
            _check(ph, W2, kw)
            for k in range(d):
                r = tuple(rng) if np.ndim(rng) == 1 else per_dim[k]
                assert np.array_equal(ph.counts[k], np.histogram(W[:, k], bins, range=r)[0])
        kw = dict(bins=bins, range=[(0.0, 1.0), (-3.0, -1.0)], dims=[6, 4])      # a subset in non-sorted order
        ph = _device(e, n_burn, **kw)
        assert np.array_equal(ph.dims, [6, 4])
        _check(ph, W, kw)
    for k, text in ((4, r"autodetected range of \[nan, nan\] is not finite"),):
        with pytest.raises(ValueError, match=text):
            _device(e, 0)
        with pytest.raises(ValueError, match=text):
            _device(e, 0, dims=[k])
    with pytest.raises(ValueError, match=r"autodetected range of \[-inf, inf\] is not finite"):
        _device(e, N * 4, dims=[4])                       # the window starts behind the NaN: NumPy names the infinities
    with pytest.raises(ValueError, match=r"autodetected range of \[-inf, .*\] is not finite"):
        _device(e, N * 6, dims=[4])
    _check(_device(e, N * 7), _window(X, N * 7), {})      # ... and behind all of them the column is fine
    e.close()


def test_dream_shuffled_history_partial_generation():
    N = 1024
    s = _dream_class(N, 100, 300)
    n_burn = N * 40 + 5
    W = s.param_est(n_burn)[2]
    ph = s.param_est_hist(n_burn)
    _check(ph, W, {})
    _invariant(ph)
    kw = dict(dims=[97, 3, 50, 0, 99, 12, 13, 64], pairs="all")
    ph = s.param_est_hist(n_burn, **kw)
    assert len(ph.pairs) == 28 and tuple(ph.pairs[0]) == (97, 3)
    _check(ph, W, kw)
    _invariant(ph)
    kw = dict(bins=50, bins2d=33, range=(-4.0, 6.5), pairs=[(99, 0), (0, 99), (5, 6)])
    _check(s.param_est_hist(n_burn, **kw), W, kw)
    assert np.array_equal(s.param_est_hist(n_burn, bins=11).density()[7], np.histogram(W[:, 7], 11, density=True)[0])


def test_demc_banana_with_snooker():
    from bipymc_amd.demc import DeMcMpi
    from bipymc_amd.utils import banana_rv
    s = DeMcMpi(banana_rv.Banana_2D().ln_like, np.zeros(2), n_chains=512, seed=99, p_snooker=0.2)
    s.run_mcmc(512 * 400)
    n_burn = 512 * 100 + 77
    W = s.param_est(n_burn)[2]
    for kw in (dict(pairs="all"), dict(bins=1024, bins2d=64, pairs=[(1, 0)]), dict(bins=1, pairs="all"),
               dict(range=(-1.0, 1.0), pairs="all", bins2d=5)):
        ph = s.param_est_hist(n_burn, **kw)
        _check(ph, W, kw)
        if kw.get("range") is None and kw.get("bins2d") is None:
            _invariant(ph)


def test_wide_rows():
    N = 64
    s = _dream_class(N, 640, 150)
    n_burn = N * 10 + 1
    W = s.param_est(n_burn)[2]
    kw = dict(pairs=[(639, 0), (300, 301), (17, 638), (255, 256)])
    ph = s.param_est_hist(n_burn, **kw)
    _check(ph, W, kw)
    _invariant(ph)
    kw = dict(bins=1024, dims=[639, 256, 255, 1])
    _check(s.param_est_hist(n_burn, **kw), W, kw)


def test_serial_demc():
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.3, dim=6)
    s = DeMc(t.ln_like, n_chains=64, seed=8)
    s.run_mcmc(64 * 300, np.zeros(6))
    n_burn = 64 * 50 + 1
    kw = dict(pairs="all")
    ph = s.param_est_hist(n_burn, **kw)
    _check(ph, s.param_est(n_burn)[2], kw)
    _invariant(ph)


def test_cfg2_size():
    """N = 8192, d = 100, 120 generations (0.8 GB of history): all marginals, a handful of pairs on the host"""
    e = _engine(8192, 100, burnin_gen=100, n_cr_gen=20)
    e.set_state(np.random.RandomState(4).normal(size=(8192, 100)) * np.sqrt(np.arange(100) + 1.0))
    e.begin_run()
    e.step(120)
    n_burn = 8192 * 20 + 100
    kw = dict(pairs=[(0, 1), (99, 0), (42, 43), (98, 99), (50, 7)])
    ph = _device(e, n_burn, **kw)
    allp = _device(e, n_burn, dims=list(range(8)), pairs="all")
    H = e.get_history()
    e.close()
    W = _window(H, n_burn)
    _check(ph, W, kw)
    _invariant(ph)
    _invariant(allp)
    assert np.array_equal(allp.counts, ph.counts[:8])
    assert np.array_equal(allp.counts2d[0], ph.counts2d[0])
    for p in (6, 27):
        a, b = allp.pairs[p]
        assert np.array_equal(allp.counts2d[p], np.histogram2d(W[:, a], W[:, b], 20, range=[allp.edges2d[a][[0, -1]], allp.edges2d[b][[0, -1]]])[0])


def test_no_side_effects():
    a = _engine(256, 12)
    a.set_state(np.random.RandomState(1).normal(size=(256, 12)))
    a.begin_run()
    a.step(100)
    kw = dict(pairs="all", dims=[0, 5, 11, 3])
    r1 = _device(a, 256 * 3 + 9, **kw)
    r2 = _device(a, 256 * 3 + 9, **kw)
    _same_bits(r1[:6], r2[:6])
    assert r1.n == r2.n
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
    edges = np.tile(np.linspace(-1.0, 1.0, 21), (4, 1))
    with pytest.raises(L.BpmError, match="call bpm_hist_range first"):
        e.hist_marginals(np.arange(4), edges)
    with pytest.raises(L.BpmError, match="call bpm_hist_range first"):
        e.hist_pairs(np.arange(4), edges, [0], [1])
    e.step(20)
    with pytest.raises(ValueError, match="n_burn must be >= 0"):
        _device(e, -1)
    with pytest.raises(ValueError, match="window is empty"):
        _device(e, 21 * 64)
    with pytest.raises(ValueError, match="window is empty"):
        _device(e, 10 ** 9)
    with pytest.raises(ValueError, match="dims"):
        _device(e, 0, dims=[0, 4])
    with pytest.raises(ValueError, match="dims"):
        _device(e, 0, dims=[1, 1])
    with pytest.raises(ValueError, match="must be in dims"):
        _device(e, 0, dims=[0, 1], pairs=[(1, 2)])
    with pytest.raises(ValueError, match=r"max must be larger than min in range parameter\."):
        _device(e, 0, range=(1.0, -1.0))
    with pytest.raises(ValueError, match="is not finite"):
        _device(e, 0, range=(0.0, np.inf))
    with pytest.raises(ValueError, match=r"bins = 1025 is outside the supported 1 \.\.\. 1024"):
        _device(e, 0, bins=1025)
    with pytest.raises(ValueError, match=r"bins2d = 65 is outside the supported 1 \.\.\. 64"):
        _device(e, 0, pairs="all", bins2d=65)
    assert e.hist_range(64 * 20 + 3)[0] == 61
    assert e.hist_marginals(np.arange(4), edges).shape == (4, 20)
    # the C entry points name their own limits
    with pytest.raises(L.BpmError, match=r"bins = 1025 is outside the supported 1 \.\.\. 1024"):
        e.hist_marginals(np.arange(4), np.tile(np.linspace(-1.0, 1.0, 1026), (4, 1)))
    with pytest.raises(L.BpmError, match=r"bins2d = 65 is outside the supported 1 \.\.\. 64"):
        e.hist_pairs(np.arange(4), np.tile(np.linspace(-1.0, 1.0, 66), (4, 1)), [0], [1])
    with pytest.raises(L.BpmError, match="coordinate out of range"):
        e.hist_marginals([4], edges[:1])
    with pytest.raises(L.BpmError, match="not in dims"):
        e.hist_pairs([0, 1], edges[:2], [0], [2])
    with pytest.raises(L.BpmError, match="non-decreasing"):
        e.hist_marginals([0], edges[:1, ::-1])
    e.step(1)
    with pytest.raises(L.BpmError, match="history changed"):
        e.hist_marginals(np.arange(4), edges)
    with pytest.raises(L.BpmError, match="history changed"):
        e.hist_pairs(np.arange(4), edges, [0], [1])
    e.hist_range(0)
    e.set_state(np.zeros((64, 4)))
    with pytest.raises(L.BpmError, match="history changed"):
        e.hist_marginals(np.arange(4), edges)
    e.close()


KW_GROUP = dict(pairs=[(0, 1), (99, 3), (3, 99), (50, 51)], bins2d=16)


def _group_histograms(R):
    from bipymc_amd import histograms as HS
    ranks, N, d = local_group(R)
    n_burn = N * 7 + N // 2 + 1                 # a partial generation that starts inside a later rank's chains
    res = HS.compute(per_rank(ranks, "hist_range"), per_rank(ranks, "hist_marginals"), per_rank(ranks, "hist_pairs"), lambda x: x, n_burn, d,
                     **KW_GROUP)
    for e in ranks:
        e.close()
    one = group_single_rank()
    ref = _device(one, n_burn, **KW_GROUP)
    H = one.get_history()
    one.close()
    return res, ref, _window(H, n_burn)


@pytest.mark.parametrize("R", [2, 4])
def test_local_group_equals_single_rank(R):
    res, ref, W = _group_histograms(R)
    _check(ref, W, KW_GROUP)
    _same_bits(res[:6], ref[:6])
    assert res.n == ref.n


def test_rank_processes_sharing_the_gpu(tmp_path):
    one, r = run_rank_processes(tmp_path, "hist")
    from _stats_worker import KW
    from bipymc_amd.histograms import PosteriorHistograms
    ph = PosteriorHistograms(np.arange(10), one["edges"], one["counts"], np.asarray(KW["pairs"]), one["edges2d"], one["counts2d"], int(one["n"]))
    _check(ph, one["chain_slice"], KW)
    for key in ("edges", "counts", "edges2d", "counts2d", "n"):
        a, b, c = r[0][key], r[1][key], one[key]
        if a.dtype == np.float64:
            a, b, c = a.view(np.uint64), b.view(np.uint64), c.view(np.uint64)
        assert np.array_equal(a, b) and np.array_equal(a, c), key
