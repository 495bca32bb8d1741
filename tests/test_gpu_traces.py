"""Per-generation trace summaries on the GPU (bpm_trace_bins / bpm_trace_chains + bipymc_amd/traces.py): min, max, counts, gen, n, best_* and
chain_* must equal NumPy on the history that get_history / get_loglike_history return; mean, sd and ll_mean lie within the derived bound
of tests/test_traces_host.py (trace_bound) of a np.longdouble evaluation -- on installed histories with a constant column, an offset of
1e8, denormals, NaN and infinities, with few long bins (several workgroups per bin), on sampler histories (DREAM in position order, DE-MC
with snooker, the serial class, wide rows), across ranks and rank processes; no side effects; errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from _history_cases import CHILD_LIMIT_S, _dream_class, _engine, group_single_rank, local_group, per_rank  # noqa: E402
from test_traces_host import check_against_numpy  # noqa: E402


def _device(eng, n_burn=0, every=1, chains=None):
    from bipymc_amd import traces as TR
    return TR.compute(eng.trace_bins, eng.trace_chains, TR.single_process_allgather, n_burn, eng.n_chains, eng.history_rows(), eng.dim,
                      every=every, chains=chains)


def _same_bits(a, b):
    assert a._fields == b._fields
    for f, x, y in zip(a._fields, a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, f
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y), f


def _installed(N=256, d=7, G=40):
    """d = 7: one padding column per row, kw = 8 and 32 rows side by side.  The last generation (the state) stays finite."""
    rs = np.random.RandomState(7)
    X = rs.normal(size=(G, N, d))
    X[:, :, 1] = 0.7                                                     # constant
    X[:, :, 2] = 1e8 + X[:, :, 2]                                        # far from the origin, unit noise: the shift
    X[:, :, 3] = rs.randint(0, 100, size=(G, N)) * (1024 * 5e-324)      # denormals
    X[3, 17, 4] = np.nan                                                 # NaN in some bins ...
    X[4, 0, 4] = np.nan                                                  # ... in the first row of one (the shift is another value)
    X[9, ::2, 4] = np.nan
    X[6, :, 4] = np.nan                                                  # ... and in all of one
    X[5, :40, 5] = np.inf
    X[8, 100:130, 5] = -np.inf
    X[11, 3, 5], X[11, 200, 5] = -np.inf, np.inf
    X[12, 0, 5] = np.inf
    return X


@pytest.fixture(scope="module")
def installed():
    X = _installed()
    G, N, d = X.shape
    e = _engine(N, d)
    e.set_history(X, X[-1])
    H, LL = e.get_history(), e.get_loglike_history()
    assert np.array_equal(H, X, equal_nan=True)
    yield e, H, LL
    e.close()


@pytest.mark.parametrize("every", [1, 3, 40, 1000])
@pytest.mark.parametrize("n_burn", [0, 3, 256 * 5 + 1])
def test_installed_history_against_numpy(installed, every, n_burn):
    e, H, LL = installed
    chains = [255, 0, 17]
    pt = _device(e, n_burn, every, chains)
    check_against_numpy(pt, H, LL, n_burn, every, chains)
    assert np.all(pt.sd[:, 1] == 0.0) and np.all(pt.mean[:, 1] == 0.7)
    assert pt.gen[0] == {0: 0, 3: 1, 256 * 5 + 1: 6}[n_burn]            # the first whole generation
    if every == 1 and n_burn == 0:
        assert np.isnan(pt.min[6, 4]) and pt.n_nan[6, 4] == 256 and pt.n_nan[9, 4] == 128 and np.isnan(pt.mean[3, 4])
        assert pt.mean[5, 5] == np.inf and pt.mean[8, 5] == -np.inf and np.isnan(pt.mean[11, 5]) and pt.max[12, 5] == np.inf


@pytest.mark.parametrize("every", [64, 32])
def test_few_long_bins_take_several_workgroups_per_bin(every):
    N, d, G = 4096, 7, 64
    rs = np.random.RandomState(3)
    X = rs.normal(size=(G, N, d)) * np.arange(1, d + 1)
    X[:, :, 2] += 1e8
    X[:, :, 3] = -1.5
    X[10:12, 1000:3000, 4] = np.nan
    X[50, 4000, 5] = -np.inf
    e = _engine(N, d)
    e.set_history(X, X[-1])
    H, LL = e.get_history(), e.get_loglike_history()
    pt = _device(e, 0, every, [4095, 0, 2048])
    check_against_numpy(pt, H, LL, 0, every, [4095, 0, 2048])
    assert len(pt.gen) == 64 // every
    _same_bits(pt, _device(e, 0, every, [4095, 0, 2048]))
    check_against_numpy(_device(e, N * 3 + 1, every), H, LL, N * 3 + 1, every)      # 60 generations: a short last bin of several parts
    e.close()


def _check_sampler(s, n_burn, every):
    N = s.n_chains
    chains = [0, N - 1, 5]
    pt = s.param_est_trace(n_burn, every=every, chains=chains)          # (first: a history in position order is put into chain order here)
    W = s.param_est(0)[2]
    G = W.shape[0] // N
    H = W.reshape(G, N, -1)
    LL = s._engine.get_loglike_history()
    assert np.array_equal(H, s._engine.get_history())
    check_against_numpy(pt, H, LL, n_burn, every, chains)
    g0 = -(-n_burn // N)
    row = g0 * N + int(np.argmax(LL[g0:].reshape(-1)))
    assert pt.best_row == row and np.array_equal(pt.best_x, W[row]) and pt.best_ll == LL.reshape(-1)[row]
    gen = np.arange(g0, G, min(every, G - g0))
    assert np.array_equal(pt.chain_x, H[gen][:, chains]) and np.array_equal(pt.chain_ll, LL[gen][:, chains])
    _same_bits(pt, s.param_est_trace(n_burn, every=every, chains=chains))
    assert np.array_equal(s.param_est(0)[2], W)
    return pt


def test_dream_shuffled_history_in_position_order():
    s = _dream_class(256, 10, 60)
    _check_sampler(s, 256 * 4 + 9, 4)
    _check_sampler(s, 0, 1)


def test_demc_banana_with_snooker():
    from bipymc_amd.demc import DeMcMpi
    from bipymc_amd.utils import banana_rv
    s = DeMcMpi(banana_rv.Banana_2D().ln_like, np.zeros(2), n_chains=512, seed=99, p_snooker=0.2)
    s.run_mcmc(512 * 100)
    _check_sampler(s, 512 * 10 + 77, 9)


def test_serial_demc():
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.3, dim=6)
    s = DeMc(t.ln_like, n_chains=64, seed=8)
    s.run_mcmc(64 * 100, np.zeros(6))
    _check_sampler(s, 64 * 5 + 1, 10)


def test_wide_rows_are_more_column_tiles():
    s = _dream_class(64, 640, 30)
    _check_sampler(s, 64 * 2 + 1, 5)


@pytest.mark.parametrize("R", [2, 4])
def test_local_group_equals_single_rank(R):
    from bipymc_amd import traces as TR
    ranks, N, d = local_group(R)
    n_burn, every = N * 7 + N // 2 + 1, 6
    chains = [N - 1, 0, N // 2 + 1]                                      # of the last, the first and a middle rank
    G = ranks[0].history_rows()
    res = TR.compute(per_rank(ranks, "trace_bins"), per_rank(ranks, "trace_chains"), lambda x: x, n_burn, N, G, d, every=every, chains=chains)
    for e in ranks:
        e.close()
    one = group_single_rank()
    ref = _device(one, n_burn, every, chains)
    H, LL = one.get_history(), one.get_loglike_history()
    one.close()
    check_against_numpy(ref, H, LL, n_burn, every, chains)
    check_against_numpy(res, H, LL, n_burn, every, chains)              # (each within the bound of the exact value, hence of each other)
    exact = [f for f in res._fields if f not in ("mean", "sd", "ll_mean")]
    _same_bits(TR.PosteriorTrace(**{f: getattr(res, f) if f in exact else 0.0 for f in res._fields}),
               TR.PosteriorTrace(**{f: getattr(ref, f) if f in exact else 0.0 for f in res._fields}))


def test_rank_processes_sharing_the_gpu(tmp_path):
    """tests/_trace_worker.py: one single-rank process, then two ranks together, every child under `timeout -k 10`; nothing more is started
    after a child that did not exit with 0"""
    from _trace_worker import KW, N_BURN
    from bipymc_amd import traces as TR
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["BPM_PUSH_TIMEOUT_S"] = "60"
    d_ = str(tmp_path)

    def child(rank, world):
        return ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(HERE, "_trace_worker.py"), d_, str(rank), str(world)]

    subprocess.check_call(child(0, 1), env=env, timeout=CHILD_LIMIT_S + 30)
    procs = [subprocess.Popen(child(r, 2), env=env) for r in range(2)]
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=CHILD_LIMIT_S + 30))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert codes == [0, 0], codes
    name = os.path.join(d_, "tr_w%d_rank%d.npz")
    one, r = np.load(name % (1, 0)), [np.load(name % (2, k)) for k in range(2)]

    def trace(z):
        return TR.PosteriorTrace(**{f: (z[f] if z[f].ndim else z[f][()]) for f in TR.PosteriorTrace._fields})

    H, LL = one["history"], one["loglike_history"]
    check_against_numpy(trace(one), H, LL, N_BURN, KW["every"], KW["chains"])
    check_against_numpy(trace(r[0]), H, LL, N_BURN, KW["every"], KW["chains"])
    for f in TR.PosteriorTrace._fields:
        a, b = r[0][f], r[1][f]
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                      b.view(np.uint64) if b.dtype == np.float64 else b), f
        if f not in ("mean", "sd", "ll_mean"):
            assert np.array_equal(a, one[f], equal_nan=True), f


def test_no_side_effects():
    a = _engine(256, 12)
    a.set_state(np.random.RandomState(1).normal(size=(256, 12)))
    a.begin_run()
    a.step(100)
    r1 = _device(a, 256 * 3 + 9, 5, [0, 255])
    r2 = _device(a, 256 * 3 + 9, 5, [0, 255])
    _same_bits(r1, r2)
    a.step(100)
    b = _engine(256, 12)
    b.set_state(np.random.RandomState(1).normal(size=(256, 12)))
    b.begin_run()
    b.step(200)
    assert np.array_equal(a.get_history(), b.get_history())
    assert np.array_equal(a.get_loglike_history(), b.get_loglike_history())
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
        with pytest.raises(L.BpmError, match="bpm_trace_bins: needs keep_history=True"):
            _device(e, 0)
        e.close()
    e = _engine(64, 4)
    e.set_state(np.random.RandomState(2).normal(size=(64, 4)))
    e.begin_run()
    with pytest.raises(L.BpmError, match="bpm_trace_chains: call bpm_trace_bins first"):
        e.trace_chains([0])
    e.step(20)
    with pytest.raises(ValueError, match=r"param_est_trace: every must be >= 1 \(got 0\)"):
        _device(e, 0, every=0)
    with pytest.raises(ValueError, match=r"param_est_trace: chains must lie in \[0, 64\)"):
        _device(e, 0, chains=[64])
    with pytest.raises(ValueError, match="param_est_trace: chains must be distinct"):
        _device(e, 0, chains=[1, 1])
    with pytest.raises(ValueError, match="param_est_trace: n_burn must be >= 0"):
        _device(e, -1)
    with pytest.raises(ValueError, match="param_est_trace: the window is empty"):
        _device(e, 20 * 64 + 1)
    with pytest.raises(ValueError, match="window is empty"):
        _device(e, 10 ** 9)
    assert len(_device(e, 20 * 64).gen) == 1
    # the C entry points name their own limits
    with pytest.raises(L.BpmError, match=r"bpm_trace_bins: every must be >= 1 \(got 0\)"):
        e.trace_bins(0, 21, 0)
    with pytest.raises(L.BpmError, match="bpm_trace_bins: generation range out of bounds"):
        e.trace_bins(0, 22, 1)
    with pytest.raises(L.BpmError, match="bpm_trace_bins: generation range out of bounds"):
        e.trace_bins(-1, 21, 1)
    e.trace_bins(0, 21, 4)
    assert e.trace_chains([63, 2])[1].shape == (6, 2, 4)
    ids = (L.C.c_int32 * 1)(64)
    buf = np.empty(6 * 4)
    with pytest.raises(L.BpmError, match=r"bpm_trace_chains: local chain 64 is outside \[0, 64\)"):
        e._ck(e.lib.bpm_trace_chains(e._h, 1, ids, buf.ctypes.data_as(L.C.POINTER(L.C.c_double)), buf.ctypes.data_as(L.C.POINTER(L.C.c_double))))
    e.step(1)
    with pytest.raises(L.BpmError, match=r"bpm_trace_chains: the history changed since bpm_trace_bins .*call it again"):
        e.trace_chains([0])
    e.trace_bins(0, 22, 4)
    e.set_state(np.zeros((64, 4)))
    with pytest.raises(L.BpmError, match="history changed since bpm_trace_bins"):
        e.trace_chains([0])
    e.close()
    from bipymc_amd.samplers import DeMc
    with pytest.raises(RuntimeError, match="param_est_trace: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).param_est_trace()
