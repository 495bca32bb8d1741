"""Thinned histories on the GPU (bpm_set_history_thin / bpm_thin_history / bpm_set_history_thinned / bpm_get_history_thin): a history of
stride k is exactly [::k] of the dense run's from the same seed and everything else -- state, ln-likes, accept counters, CR statistics -- is
the dense run's, bit for bit, on every append path; thin_history on a dense run; every statistic over a thinned handle; the moment rebuild of
a second DREAM run; the checkpoint; the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from _memory_cases import _free_device_memory, _over  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), what


# ---- the cases: the smallest shapes that between them reach every append path -------------------------------------------------------------
def _spec(name, d):
    from bipymc_amd.utils import banana_rv, d100_gauss, mixture_nd
    if name == "gauss":
        return d100_gauss.Gauss_100D(rho=0.5, dim=d)._bpm_target_spec()
    if name == "mixture":
        return mixture_nd.BimodeGauss_ND(d)._bpm_target_spec()
    return banana_rv.Banana_2D()._bpm_target_spec()


def _case(case):
    """-> (algo, target, d, N, engine kwargs, run options, generations, k)"""
    from bipymc_amd import _lib as L
    return {
        # plan records, burn-in into the steady state, crosses the 64-generation table window
        "dream_gauss100": (L.ALGO_DREAM, "gauss", 100, 32, dict(burnin_gen=10, n_cr_gen=4), {}, 70, 3),
        # 4 lanes per chain, position-ordered append
        "dream_mix8": (L.ALGO_DREAM, "mixture", 8, 64, dict(burnin_gen=8, n_cr_gen=3), {}, 30, 4),
        # one lane per chain, lean
        "demc_banana": (L.ALGO_DEMC, "banana", 2, 128, dict(p_snooker=0.1), {}, 21, 2),
        # the looped kernel
        "dream_gauss640": (L.ALGO_DREAM, "gauss", 640, 24, dict(burnin_gen=6, n_cr_gen=2), {}, 10, 3),
        # synchronous DE-MC (the serial class's run options)
        "demc_sync": (L.ALGO_DEMC_SYNC, "gauss", 100, 24, {}, dict(shuffle=False, flip=0.0), 10, 3),
    }[case]


def _x0(N, d):
    return np.random.RandomState(3).normal(size=(N, d)) + 0.5


def _engine(case, thin=1, **more):
    from bipymc_amd.engine import HipEngine
    algo, target, d, N, kw, ropts, G, k = _case(case)
    tid, tp, _ = _spec(target, d)
    e = HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, thin=thin, **dict(kw, **more))
    e.set_state(_x0(N, d))
    e.begin_run(**ropts)
    return e


def _pieces(G):
    return [p for p in (7, 1, G - 8) if p > 0] if G > 8 else [G]


def _snapshot(e):
    st = e.stats()
    return dict(hist=e.get_history(), llhist=e.get_loglike_history(), state=e.get_state(), ll=e.get_loglike(),
                counts=np.array([st["local_n_accepted"], st["local_n_rejected"], st["n_nan_alpha"]], dtype=np.float64),
                p_cr=st["p_cr"], delta_m=st["delta_m"], n_cr_updates=st["n_cr_updates"])


def _thinned_equals_dense(thin_snap, dense_snap, k, what):
    _same(thin_snap["hist"], dense_snap["hist"][::k], what + ": history")
    _same(thin_snap["llhist"], dense_snap["llhist"][::k], what + ": ln-like history")
    for key in ("state", "ll", "counts", "p_cr", "delta_m", "n_cr_updates"):
        _same(thin_snap[key], dense_snap[key], what + ": " + key)


def _thin_numbers(G, k):
    return dict(thin=k, rows_logical=G + 1, rows=G // k + 1, last_stored=(G // k) * k)


_DENSE = {}


def _dense(case):
    """the dense twin of a case, run once for the tests that compare with it: its snapshots after the first G0 and after all generations"""
    if case not in _DENSE:
        G = _case(case)[6]
        e = _engine(case)
        for p in _pieces(G):
            e.step(p)
        first = _snapshot(e)
        e.step(13)
        _DENSE[case] = (first, _snapshot(e))
        e.close()
    return _DENSE[case]


# ---- 1. a thinned run against its dense twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dream_gauss100", "dream_mix8", "demc_banana", "dream_gauss640", "demc_sync"])
def test_thinned_run_is_every_kth_row_of_the_dense_run(case):
    G, k = _case(case)[6:8]
    e = _engine(case, thin=k)
    assert e.history_thin() == _thin_numbers(0, k)
    done = 0
    for p in _pieces(G):
        e.step(p)
        done += p
        assert e.history_thin() == _thin_numbers(done, k)
    _thinned_equals_dense(_snapshot(e), _dense(case)[0], k, case)
    e.close()


def _py_ll(X):
    return -0.5 * np.sum(np.asarray(X) ** 2, axis=-1)


def test_thinned_host_callback_run_through_propose_and_commit():
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    N, d, k, G = 8, 5, 2, 11                      # (11 generations: the last one is not stored)
    snaps = []
    for thin in (1, k):
        e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=11, burnin_gen=6, n_cr_gen=2,
                      thin=thin)
        e.set_state(_x0(N, d))
        e.set_loglike(_py_ll(_x0(N, d)))
        e.begin_run()
        for _ in range(G):
            for _half in range(2):
                props, _ids = e.propose()
                e.commit(_py_ll(props))
        if thin > 1:
            assert e.history_thin() == _thin_numbers(G, k)
        snaps.append(_snapshot(e))
        e.close()
    _thinned_equals_dense(snaps[1], snaps[0], k, "host callback")


_HIP_SRC = """
#define BPM_LN_LIKE_TERMS 1
__device__ void ln_like_terms(double xj, int j, int d, const double* p, double* acc) { const double z = (xj - p[j]) * p[d + j]; acc[0] += z * z; }
__device__ double ln_like_finish(const double* acc, int d, const double* p) { return -0.5 * acc[0]; }
"""


def test_thinned_run_with_a_hip_source_likelihood_in_the_fused_form():
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    N, d, k, G = 24, 100, 3, 20
    snaps = []
    for thin in (1, k):
        e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=11, burnin_gen=8, n_cr_gen=2,
                      thin=thin)
        e.set_state(_x0(N, d))
        e.set_device_likelihood(_HIP_SRC, np.concatenate([np.linspace(-1, 1, d), 1.0 / (1.0 + np.arange(d) % 3)]))
        fused, why = e.device_likelihood_info()
        assert fused, why
        e.begin_run()
        for p in _pieces(G):
            e.step(p)
        snaps.append(_snapshot(e))
        e.close()
    _thinned_equals_dense(snaps[1], snaps[0], k, "HIP-source likelihood")


def test_two_ranks_over_the_push_exchange_store_the_dense_runs_rows():
    """tests/_history_cases.py's local group (the test variant's ranks of one process), thinned: each rank's rows are its block of the dense
    single-rank run's [::3]"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    R, N, d, k, G = 2, 32, 100, 3, 20
    tid, tp, _ = d100_gauss.Gauss_100D()._bpm_target_spec()
    kw = dict(burnin_gen=8, n_cr_gen=3)
    one = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, **kw)
    one.set_state(_x0(N, d))
    one.begin_run(flip=0.4)
    one.step(G)
    dense = _snapshot(one)
    one.close()
    uid = b"BPMLOCAL" + bytes(120)
    lib = L.load_test()
    ranks = [HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, rank=r, world_size=R, nccl_uid=uid, lib=lib,
                       thin=k, **kw) for r in range(R)]
    blobs = [e.push_export() for e in ranks]
    for e in ranks:
        e.push_connect(blobs)
    arr = (C.c_void_p * R)(*[e._h for e in ranks])
    ok = C.c_int32(0)
    L.check(lib.bpm_push_selftest(arr, R, C.byref(ok)), lib)
    assert ok.value == 1
    for e in ranks:
        e.set_state(_x0(N, d))
        e.begin_run(flip=0.4)
    for p in _pieces(G):
        L.check(lib.bpm_local_group_step(arr, R, p), lib)
    n_local = N // R
    for r, e in enumerate(ranks):
        assert e.history_thin() == _thin_numbers(G, k)
        _same(e.get_history(), dense["hist"][::k, r * n_local:(r + 1) * n_local], "rank %d: history" % r)
        _same(e.get_loglike_history(), dense["llhist"][::k, r * n_local:(r + 1) * n_local], "rank %d: ln-like history" % r)
        _same(e.get_state(), dense["state"], "rank %d: state" % r)
        _same(e.stats()["p_cr"], dense["p_cr"], "rank %d: p_cr" % r)
    for e in ranks:
        e.close()


# ---- 2. thin_history on a dense run -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dream_gauss100", "dream_mix8", "demc_banana"])       # (the last two carry position-order tags)
def test_thin_history_on_a_dense_run_and_going_on(case):
    from bipymc_amd._lib import BpmError
    from bipymc_amd import quantiles as Q
    G = _case(case)[6]
    first, later = _dense(case)
    e = _engine(case)
    for p in _pieces(G):
        e.step(p)
    e.quantile_begin(0)                               # a snapshot of the history as it is
    e.thin_history(1)                                 # a no-op: the same epoch, the snapshot still answers
    e.quantile_histogram([0], [0], 0)
    assert e.history_thin() == _thin_numbers(G, 1)
    e.thin_history(4)
    assert e.history_thin() == _thin_numbers(G, 4)
    with pytest.raises(BpmError, match="history changed"):
        e.quantile_histogram([0], [0], 0)
    _thinned_equals_dense(_snapshot(e), first, 4, case + ": after thin_history(4)")
    e.step(13)
    assert e.history_thin() == _thin_numbers(G + 13, 4)
    _thinned_equals_dense(_snapshot(e), later, 4, case + ": 13 generations later")
    # the quantiles of what is stored: np.quantile over the dense twin's every fourth row
    got = Q.compute(e.quantile_begin, e.quantile_histogram, Q.single_process_allgather, 0, [0.05, 0.5, 0.95], dim=e.dim)
    H = later["hist"][::4]
    assert np.array_equal(got, np.quantile(H.reshape(-1, H.shape[-1]), [0.05, 0.5, 0.95], axis=0))
    e.close()


def _installed(N, d, rows):
    """a host-callback engine with `rows` random history rows and known ln-likes in the last one"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    H = np.random.RandomState(rows).normal(size=(rows, N, d))
    e = HipEngine(algo=L.ALGO_DEMC, n_chains=N, dim=d, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=2)
    e.set_history(H, H[-1])
    e.set_loglike(_py_ll(H[-1]))
    return e, H


def test_thin_history_edge_shapes():
    # N = 5, d = 1: an odd number of ln-likes per row (8-byte accesses), the smallest state row; rows - 1 = 10 is no multiple of 4
    e, H = _installed(5, 1, 11)
    ll = e.get_loglike_history()
    e.thin_history(4)
    assert e.history_thin() == dict(thin=4, rows_logical=11, rows=3, last_stored=8)
    _same(e.get_history(), H[::4], "N = 5, d = 1")
    _same(e.get_loglike_history(), ll[::4], "N = 5, d = 1: ln-likes")
    e.close()
    # 3 then 2: stride 6
    e, H = _installed(6, 3, 20)
    ll = e.get_loglike_history()
    e.thin_history(3)
    e.thin_history(2)
    assert e.history_thin() == dict(thin=6, rows_logical=20, rows=4, last_stored=18)
    _same(e.get_history(), H[::6], "3 then 2")
    _same(e.get_loglike_history(), ll[::6], "3 then 2: ln-likes")
    # m beyond the row count: one row is left, and recording goes on aligned
    e.thin_history(1000)
    assert e.history_thin() == dict(thin=6000, rows_logical=20, rows=1, last_stored=0)
    _same(e.get_history(), H[:1], "m beyond the row count")
    e.close()


def test_thin_history_returns_the_memory():
    """N = 4096, d = 100, 200 generations, m = 4: three quarters of the old history's bytes are due back; half are asserted (allocator
    granularity)"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    N, d, G = 4096, 100, 200
    tid, tp, _ = _spec("gauss", d)
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, burnin_gen=10, n_cr_gen=4)
    e.set_state(_x0(N, d))
    e.begin_run()
    e.step(G)
    e.synchronize()
    old_bytes = (G + 1) * N * (d + 1) * 8
    before = _free_device_memory()
    e.thin_history(4)
    after = _free_device_memory()
    print("history %d bytes; free memory rose by %d" % (old_bytes, after - before))
    assert after - before >= old_bytes // 2
    assert e.history_thin() == _thin_numbers(G, 4)
    e.close()


# ---- 3. every statistic over a thinned handle ---------------------------------------------------------------------------------------------------
def _walk(obj, path="result"):
    """every array / number inside a statistic's result, with its path"""
    if isinstance(obj, (np.ndarray, float, int, np.floating, np.integer)) or obj is None:
        yield path, obj
    elif isinstance(obj, dict):
        for k in sorted(obj):
            for it in _walk(obj[k], "%s[%r]" % (path, k)):
                yield it
    elif isinstance(obj, (list, tuple)) and not hasattr(obj, "_fields"):
        for i, v in enumerate(obj):
            for it in _walk(v, "%s[%d]" % (path, i)):
                yield it
    elif hasattr(obj, "_asdict"):
        for it in _walk(dict(obj._asdict()), path):
            yield it
    elif hasattr(obj, "__dict__"):
        for it in _walk({k: v for k, v in vars(obj).items() if not k.startswith("_")}, path):
            yield it
    else:
        yield path, obj


def _same_result(a, b, what):
    la, lb = list(_walk(a)), list(_walk(b))
    assert [p for p, _ in la] == [p for p, _ in lb], what
    assert len(la) > 0, what
    for (p, x), (_, y) in zip(la, lb):
        if isinstance(x, (np.ndarray, float, np.floating)):
            _same(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), "%s: %s" % (what, p))
        else:
            assert x == y, "%s: %s" % (what, p)


_DERIVE_SRC = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[0] + x[2] * p[0];
    out[1] = x[1] * x[5] + ll;
}"""


@pytest.fixture(scope="module")
def thinned_and_installed():
    """d = 6, N = 16, 60 generations at stride 3 -- and a dense handle into which the thinned one's get_history() was installed"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    N, d, G, k = 16, 6, 60, 3
    tid, tp, _ = _spec("gauss", d)
    kw = dict(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, burnin_gen=10, n_cr_gen=4)
    a = HipEngine(thin=k, **kw)
    a.set_state(_x0(N, d))
    a.begin_run()
    a.step(G)
    assert a.history_thin() == _thin_numbers(G, k)
    b = HipEngine(**kw)
    b.set_history(a.get_history(), a.get_state())
    assert b.history_thin() == dict(thin=1, rows_logical=G // k + 1, rows=G // k + 1, last_stored=G // k)
    yield _over(a), _over(b), N
    a.close()
    b.close()


@pytest.mark.parametrize("stat", ["moments", "quantiles", "cov", "hist", "trace", "fn", "diagnostics", "diagnostics_rank", "derived_history"])
def test_statistics_over_a_thinned_handle_equal_those_over_its_rows_installed(thinned_and_installed, stat):
    from bipymc_amd.derived import HipFunction
    a, b, N = thinned_and_installed
    n_burn = 3 * N + 5                       # (stored rows: a partial first generation)
    fn = HipFunction(_DERIVE_SRC, n_out=2, params=[0.25])

    def run(o):
        eng = o._stats_engine("test")
        if stat == "moments":
            return eng.reduce_moments(n_burn)
        if stat == "quantiles":
            return o.param_est_quantiles(n_burn, q=[0.0, 0.05, 0.5, 0.95, 1.0])
        if stat == "cov":
            return o.param_est_cov(n_burn)
        if stat == "hist":
            return o.param_est_hist(n_burn, bins=12, pairs="all", bins2d=5)
        if stat == "trace":
            return o.param_est_trace(n_burn, every=4, chains=[0, 7])
        if stat == "fn":
            return o.param_est_fn(fn, n_burn, values=True)
        if stat == "diagnostics":
            return o.convergence_diagnostics(n_burn)
        if stat == "diagnostics_rank":
            return o.convergence_diagnostics_rank(n_burn)
        with o.derived_history(fn) as dh:
            eng2 = dh._stats_engine("test")
            assert eng2.history_thin()["thin"] == 1 and eng2.history_rows() == eng.history_rows()      # an ordinary stride-1 history of the stored rows
            return eng2.get_history(), eng2.get_loglike_history(), dh.param_est_quantiles(n_burn), dh.convergence_diagnostics(0)

    _same_result(run(a), run(b), stat)


# ---- 4. a second run on a thinned DreamMpi ------------------------------------------------------------------------------------------------------
def test_second_run_of_a_thinned_dream_rebuilds_its_moments_from_the_stored_rows(monkeypatch):
    import bipymc_amd.demc as D
    from bipymc_amd import DreamMpi, _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    monkeypatch.setattr(D, "_engine_factory", lambda **kw: HipEngine(lib=L.load_test(), **kw))
    N, d, k = 16, 6, 3
    t = d100_gauss.Gauss_100D(rho=0.5, dim=d)
    s = DreamMpi(t.ln_like, np.zeros(d), n_chains=N, n_cr_gen=4, burnin_gen=10, seed=21, thin=k)
    s.run_mcmc(N * (20 + 1))                              # 20 generations, the last 10 without adaptation: logical rows 0 .. 20, stored 0, 3, ..., 18
    eng = s._engine
    assert eng.history_thin() == _thin_numbers(20, k)
    H = eng.get_history()
    assert len(H) == 7
    s.run_mcmc(N * (1 + 1))                               # a second run: k_gen starts again, CR adaptation is on and rebuilds its moments
    assert eng.history_thin() == _thin_numbers(21, k)
    x_new = eng.get_state()
    # the same recurrences in the same order: the stored rows, the scale, one Welford step counted with rows_logical
    mean, m2 = np.zeros((N, d)), np.zeros((N, d))
    for g in range(len(H)):
        d1 = H[g] - mean
        mean = mean + d1 / float(g + 1)
        m2 = m2 + d1 * (H[g] - mean)
    m2 = m2 * (21.0 / 7.0)
    d1 = x_new - mean
    mean = mean + d1 / float(21 + 1)
    m2 = m2 + d1 * (x_new - mean)
    got_mean, got_m2 = eng.debug_welford()
    np.testing.assert_allclose(got_mean, mean, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got_m2, m2, rtol=1e-12, atol=0)
    p_cr = np.asarray(s.p_cr)
    assert np.all(np.isfinite(p_cr)) and abs(p_cr.sum() - 1.0) < 1e-12
    assert s.thin == k and np.array_equal(s.history_generations(), np.arange(8) * k)


# ---- 5. checkpoint round trip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [".h5", ".npz"])
def test_checkpoint_of_a_thinned_sampler_round_trips(tmp_path, ext):
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    N, d, k = 16, 6, 3
    t = d100_gauss.Gauss_100D(rho=0.5, dim=d)
    kw = dict(n_chains=N, n_cr_gen=4, burnin_gen=10, seed=21)
    s = DreamMpi(t.ln_like, np.zeros(d), thin=k, **kw)
    s.run_mcmc(N * (20 + 1))                              # logical row 20 is not stored
    path = str(tmp_path / ("ck" + ext))
    s.save_state(path)
    H, X = s._engine.get_history(), s._engine.get_state()
    assert not np.array_equal(H[-1], X)
    w = DreamMpi(t.ln_like, np.zeros(d), thin=k, **kw)
    w.load_state(path)
    assert w.thin == k and w._engine.history_thin() == _thin_numbers(20, k)
    _same(w._engine.get_history(), H, "history")
    _same(w._engine.get_state(), X, "current state")
    _same(w._engine.get_loglike(), s._engine.get_loglike(), "ln-likes of the current state")
    w.run_mcmc(N * (4 + 1))                               # ... and goes on, recording aligned: logical rows 21 and 24 are stored
    assert w._engine.history_thin() == _thin_numbers(24, k)
    # a multiple of the file's stride thins further; anything else is refused
    w6 = DreamMpi(t.ln_like, np.zeros(d), thin=2 * k, **kw)
    w6.load_state(path)
    assert w6._engine.history_thin() == _thin_numbers(20, 2 * k)
    _same(w6._engine.get_history(), H[::2], "thinned further")
    _same(w6._engine.get_state(), X, "current state, thinned further")
    w2 = DreamMpi(t.ln_like, np.zeros(d), thin=2, **kw)
    with pytest.raises(ValueError, match="multiple"):
        w2.load_state(path)
    # a file as the parent's code wrote it: no thinning fields
    from bipymc_amd import checkpoint
    dense = DreamMpi(t.ln_like, np.zeros(d), **kw)
    dense.run_mcmc(N * (9 + 1))
    Hd = dense._engine.get_history()
    old = str(tmp_path / ("old" + ext))
    checkpoint.write(old, Hd, dict(t_abs=9, seed=21))
    o = DreamMpi(t.ln_like, np.zeros(d), **kw)
    o.load_state(old)
    assert o._engine.history_thin() == _thin_numbers(9, 1)
    _same(o._engine.get_history(), Hd, "a file without the fields")
    _same(o._engine.get_state(), Hd[-1], "its state is its last row")
    o4 = DreamMpi(t.ln_like, np.zeros(d), thin=4, **kw)
    o4.load_state(old)
    assert o4._engine.history_thin() == _thin_numbers(9, 4)
    _same(o4._engine.get_history(), Hd[::4], "a file without the fields, thinned on loading")


def test_checkpoint_with_one_stored_row_keeps_the_initial_row_and_the_current_state(tmp_path):
    """fewer generations than the stride: the one stored row is the INITIAL state, the current state is another -- both come back"""
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    N, d, k = 16, 6, 10
    t = d100_gauss.Gauss_100D(rho=0.5, dim=d)
    kw = dict(n_chains=N, n_cr_gen=2, burnin_gen=4, seed=21, thin=k)
    s = DreamMpi(t.ln_like, np.zeros(d), **kw)
    s.run_mcmc(N * (5 + 1))
    assert s._engine.history_thin() == dict(thin=k, rows_logical=6, rows=1, last_stored=0)
    H, LH, X = s._engine.get_history(), s._engine.get_loglike_history(), s._engine.get_state()
    assert not np.array_equal(H[0], X)
    for ext in (".h5", ".npz"):
        path = str(tmp_path / ("one" + ext))
        s.save_state(path)
        w = DreamMpi(t.ln_like, np.zeros(d), **kw)
        w.load_state(path)
        assert w._engine.history_thin() == dict(thin=k, rows_logical=6, rows=1, last_stored=0)
        _same(w._engine.get_history(), H, ext + ": row 0")
        _same(w._engine.get_loglike_history(), LH, ext + ": ln-likes of row 0")
        _same(w._engine.get_state(), X, ext + ": current state")
        _same(w._engine.get_loglike(), s._engine.get_loglike(), ext + ": ln-likes of the current state")
        w.run_mcmc(N * (5 + 1))                           # logical row 10 is stored, recording aligned
        assert w._engine.history_thin() == _thin_numbers(10, k)
        _same(w._engine.get_history()[0], H[0], ext + ": row 0 after going on")


def test_single_row_warm_start_on_the_engine_with_a_host_callback_target():
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    N, d = 8, 5
    rs = np.random.RandomState(4)
    H, X = rs.normal(size=(1, N, d)), rs.normal(size=(N, d))
    e = HipEngine(algo=L.ALGO_DEMC, n_chains=N, dim=d, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=2)
    e.set_history(H, X, thin=4, rows_logical=3)
    e.set_loglike(_py_ll(X))                              # the current state's: the stored row is not the state, its ln-likes stay unknown
    assert e.history_thin() == dict(thin=4, rows_logical=3, rows=1, last_stored=0)
    _same(e.get_history(), H, "row 0")
    _same(e.get_state(), X, "state")
    assert np.all(np.isnan(e.get_loglike_history()))
    _same(e.get_loglike(), _py_ll(X), "ln-likes of the state")
    e.set_history(H, H[0], thin=4, rows_logical=1)        # ... and where the one row IS the state, bpm_set_loglike fills it
    e.set_loglike(_py_ll(H[0]))
    _same(e.get_loglike_history()[0], _py_ll(H[0]), "ln-likes of row 0")
    e.close()


def test_param_est_moments_of_a_thinned_sampler_class():
    """the class-level method: over a thinned DreamMpi it equals, bit for bit, the same call over a dense one holding the stored rows, and
    param_est's own mean and std over them"""
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    N, d, k = 16, 6, 3
    t = d100_gauss.Gauss_100D(rho=0.5, dim=d)
    kw = dict(n_chains=N, n_cr_gen=4, burnin_gen=10, seed=21)
    s = DreamMpi(t.ln_like, np.zeros(d), thin=k, **kw)
    s.run_mcmc(N * (31 + 1))                              # logical row 31 is not stored
    b = DreamMpi(t.ln_like, np.zeros(d), **kw)
    b._engine.set_history(s._engine.get_history(), s._engine.get_state())
    for n_burn in (0, 2 * N + 3, 5 * N):
        got, want = s.param_est_moments(n_burn), b.param_est_moments(n_burn)
        _same(got[0], want[0], "mean")
        _same(got[1], want[1], "std")
        mean, std, rows = s.param_est(n_burn)
        assert rows.shape == (11 * N - n_burn, d)
        np.testing.assert_allclose(got[0], mean, rtol=1e-11, atol=1e-13)      # (the bounds the dense method is held to against param_est: test_gpu_api.py)
        np.testing.assert_allclose(got[1], std, rtol=1e-9)


# ---- 6. refusals, each by message ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from bipymc_amd import _lib as L
    from bipymc_amd._lib import BpmError
    from bipymc_amd.engine import HipEngine
    N, d = 16, 6
    tid, tp, _ = _spec("gauss", d)
    kw = dict(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, burnin_gen=10, n_cr_gen=4)
    e = HipEngine(**kw)
    e.set_state(_x0(N, d))
    with pytest.raises(BpmError, match="at least 1"):
        e.set_history_thin(0)
    with pytest.raises(BpmError, match="at least 1"):
        e.thin_history(0)
    e.set_history_thin(3)
    e.set_state(_x0(N, d))                              # the stride belongs to the handle
    assert e.history_thin()["thin"] == 3
    e.begin_run()
    e.step(4)
    e.set_history_thin(3)                               # the current stride: allowed
    with pytest.raises(BpmError, match="bpm_thin_history"):
        e.set_history_thin(2)                           # the history already has rows
    H = np.random.RandomState(0).normal(size=(4, N, d))
    with pytest.raises(BpmError, match="do not agree"):
        e.set_history(H, H[-1], thin=3, rows_logical=13)
    assert e.history_thin() == _thin_numbers(4, 3)      # (refused before anything changed)
    e.set_history(H, H[-1], thin=3, rows_logical=12)
    assert e.history_thin() == dict(thin=3, rows_logical=12, rows=4, last_stored=9)
    e.close()
    for extra, word in ((dict(keep_history=False), "keeps no history"), (dict(running_moments=True), "running_moments"),
                        (dict(outlier_every=5), "outlier")):
        with pytest.raises(BpmError, match=word):
            HipEngine(thin=2, **dict(kw, **extra))
        e = HipEngine(**dict(kw, **extra))
        e.set_state(_x0(N, d))
        e.set_history_thin(1)                           # stride 1 changes nothing, whatever the handle keeps
        e.thin_history(1)
        with pytest.raises(BpmError, match=word):
            e.thin_history(2)
        e.close()


def test_a_reservation_beyond_the_free_memory_is_refused_with_advice():
    from bipymc_amd._lib import BpmError
    e = _engine("dream_gauss100")
    row_bytes = e.n_local * (e.dim + 1) * 8
    free = _free_device_memory()
    with pytest.raises(BpmError) as err:
        e.reserve_history(2 * free // row_bytes)
    msg = str(err.value)
    assert "thin" in msg and "keep_history=False" in msg and "running_moments" in msg and "MiB" in msg
    assert abs(_free_device_memory() - free) < (64 << 20)      # nothing was allocated
    e.step(5)                                                  # the handle still steps
    assert e.history_rows() == 6
    e.close()
