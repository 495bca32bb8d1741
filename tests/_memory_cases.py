"""The cases of tests/test_gpu_device_memory.py -- the smallest configurations that between them take every allocation branch of bpm_create,
every buffer that grows and the second handle of derived_history / rank_history -- and, run as a program, the readings of the free device
memory around each of them:

    python tests/_memory_cases.py OUT.json

Every case(check=False) creates, runs and closes; check=True also compares with a twin (see the test file)."""
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _history_cases import _over  # noqa: E402,F401  (the statistics' host class over a bare engine; tests/test_gpu_history_thin.py takes it from here)


def _free_device_memory():
    """hipMemGetInfo of the runtime the library runs on (the engines' calls end in a synchronise)"""
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


N, D, G = 8, 3, 12         # d odd: ld = 4, one padding column
DERIVE_SRC = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[0] + x[2];
    out[1] = x[1] * p[0] + ll;
}"""


def _gauss(algo=None, n=N, d=D, **kw):
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, _ = d100_gauss.Gauss_100D(rho=0.5, dim=d)._bpm_target_spec()
    return HipEngine(algo=L.ALGO_DREAM if algo is None else algo, n_chains=n, dim=d, target_id=tid, target_params=tp, seed=5, **kw)


def _x0(n=N, d=D):
    return np.random.RandomState(3).normal(size=(n, d))


def _started(**kw):
    e = _gauss(**kw)
    e.set_state(_x0(e.n_chains, e.dim))
    e.begin_run()
    return e


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


def _same_sampler(a, b):
    _same(a.get_state(), b.get_state(), "state")
    _same(a.get_loglike(), b.get_loglike(), "ln-likes")
    if a.history_rows() > 1:
        _same(a.get_history(), b.get_history(), "history")
        _same(a.get_loglike_history(), b.get_loglike_history(), "ln-like history")


# ---- create, a short run, close: every allocation branch of bpm_create -------------------------------------------------------------------
def _dream_everything():
    e = _started(burnin_gen=40, n_cr_gen=5, outlier_every=10, running_moments=True, keep_history=True)
    e.step(30)
    e.close()


def _demc_sync():
    from bipymc_amd import _lib as L
    e = _started(algo=L.ALGO_DEMC_SYNC)
    e.step(6)
    e.close()


def _host_callback():
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine

    def ll(X):
        return -0.5 * np.sum(np.asarray(X) ** 2, axis=1)

    e = HipEngine(algo=L.ALGO_DEMC, n_chains=N, dim=D, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=7)
    e.set_state(_x0())
    e.set_loglike(ll(_x0()))
    e.begin_run()
    props, _ids = e.propose()
    e.commit(ll(props))
    pieces = [(k, rows.copy()) for k, rows, _ids in e.propose_chunks(2)]
    for k, rows in pieces:
        e.commit_chunk(k, ll(rows))
    e.commit_end()
    e.close()


def _local_group():
    """two ranks as handles of this process: the arena and its control block, the packed blocks, checkpoints and accept bytes, and -- under
    the push exchange the group takes once connected -- the per-chunk counts that a window's build allocates on first use"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, d = d100_gauss.Gauss_100D()._bpm_target_spec()
    R, n = 2, 32
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=L.ALGO_DREAM, n_chains=n, dim=d, target_id=tid, target_params=tp, seed=11, rank=r, world_size=R, nccl_uid=uid,
                       lib=L.load_test(), burnin_gen=2, n_cr_gen=1, outlier_every=1) for r in range(R)]
    blobs = [e.push_export() for e in ranks]
    for e in ranks:
        e.push_connect(blobs)
    arr = (C.c_void_p * R)(*[e._h for e in ranks])
    ok = C.c_int32(0)
    L.check(ranks[0].lib.bpm_push_selftest(arr, R, C.byref(ok)), ranks[0].lib)
    assert ok.value == 1
    x0 = _x0(n, d)
    for e in ranks:
        e.set_state(x0)
        e.begin_run()
    L.check(ranks[0].lib.bpm_local_group_step(arr, R, 4), ranks[0].lib)
    assert ranks[0].exchange_stats()["push_gens"] > 0
    for mode, counter in (("rows", "chunks"), ("replay", "replay_gens")):
        for e in ranks:
            e.set_exchange(mode=mode)
        L.check(ranks[0].lib.bpm_local_group_step(arr, R, 3), ranks[0].lib)
        assert ranks[0].exchange_stats()[counter] > 0
    for e in ranks:
        e.close()


def _wide_rows():
    e = _started(d=2500, burnin_gen=2, n_cr_gen=1)
    e.step(3)
    e.close()


# ---- every buffer that grows -------------------------------------------------------------------------------------------------------------
def _history_grows(check=False):
    a = _started(burnin_gen=4, n_cr_gen=2)
    b = _started(burnin_gen=4, n_cr_gen=2) if check else None
    if check:
        b.reserve_history(64)
    for n in (5, 9):           # 1 row -> 6 (the first step's capacity) -> 15 (above 6 + 6 / 2): the second step grows it, six rows kept
        a.step(n)
        if check:
            b.step(n)
            assert a.history_rows() == b.history_rows()
            _same_sampler(a, b)
    a.close()
    if check:
        b.close()


def _running_sums_grow(check=False):
    kw = dict(burnin_gen=4, n_cr_gen=2, running_moments=True, keep_history=False)
    a = _started(**kw)
    a.step(600)                # 1024 rows from the start; the second step needs 1101: grown with 601 rows kept
    a.step(500)
    if check:
        b = _started(**kw)
        b.step(1100)           # grown in front of the first generation
        for n_burn in (0, N * 600, N * 601):
            ra, rb = a.reduce_moments(n_burn), b.reduce_moments(n_burn)
            assert ra[0] == rb[0] > 0
            for x, y in zip(ra[1:], rb[1:]):
                _same(x, y, "running sums from %d" % n_burn)
        b.close()
    a.close()


def _outlier_keys_grow(check=False):
    kw = dict(burnin_gen=1000, n_cr_gen=10, outlier_every=100)
    a = _started(**kw)
    a.step(150)                # the check at generation 100: keys for 256 rows
    a.step(300)                # ... at 300: 301 rows, grown; at 400 they fit again
    if check:
        b = _started(**kw)
        b.step(450)
        assert a.stats()["n_outlier_resets"] == b.stats()["n_outlier_resets"]
        _same_sampler(a, b)
        b.close()
    a.close()


def _installed():
    X = np.random.RandomState(9).normal(size=(G, N, D))
    e = _gauss()
    e.set_history(X, X[-1])
    return e, X


def _statistics_scratch_grows(check=False):
    def quantiles(e, dims):
        e.quantile_begin(0)
        return e.quantile_histogram(dims, [0] * len(dims), 0)

    def autocov(e, lags):
        e.diag_split_moments(0, G)
        return e.diag_autocov(0, lags)

    a, _X = _installed()
    small, large = quantiles(a, [1]), quantiles(a, [0, 1, 2])        # the second request needs three times the scratch
    again = quantiles(a, [1])
    c2, c5 = autocov(a, 2), autocov(a, 5)
    if check:
        b, _X = _installed()
        large_b, small_b = quantiles(b, [0, 1, 2]), quantiles(b, [1])
        c5_b, c2_b = autocov(b, 5), autocov(b, 2)
        for x, y in zip(small + large + again + (c2, c5), small_b + large_b + small_b + (c2_b, c5_b)):
            _same(x.astype(np.float64), y.astype(np.float64), "statistics")
        b.close()
    a.close()


def _trace_on_and_off(check=False):
    from bipymc_amd import _lib as L
    a = _started(lib=L.load_test(), burnin_gen=4, n_cr_gen=2)
    a.set_trace(True)
    a.step(3)
    assert a.get_trace()["accepted"].shape == (N,)
    a.set_trace(False)
    a.step(3)
    if check:
        b = _started(lib=L.load_test(), burnin_gen=4, n_cr_gen=2)
        b.step(6)
        _same_sampler(a, b)
        b.close()
    a.close()


# ---- the second handle of derived_history / rank_history: a fresh one and one filled again ----------------------------------------------
def _derived_history(check=False):
    from bipymc_amd import HipFunction

    def py(X, ll, p):
        return np.stack([X[:, 0] + X[:, 2], X[:, 1] * p[0] + ll], axis=1)

    fn = HipFunction(DERIVE_SRC, n_out=2, params=[0.5], python_fn=py)
    e, _X = _installed()
    s = _over(e)
    with s.derived_history(fn) as dh:
        if check:
            from test_gpu_derived_history import _check_values, _values
            V, LL = _values(s, fn), e.get_loglike_history()
            assert V.shape == (G, N, 2)
            _check_values(dh, V, LL)
        e._ck(e.lib.bpm_derive_history(e._h, dh._engine._h))          # the same destination again
        if check:
            _check_values(dh, V, LL)
    e.close()


def _rank_history(check=False):
    e, X = _installed()
    s = _over(e)
    with s.rank_history(scale="rank") as rh:
        if check:
            import _rank_restatement as RR
            want = RR.restate(X)["rank"]
            assert np.array_equal(rh._engine.get_history(), want)
        e.rank_history(0, G, 0, dst=rh._engine)                        # the same destination again
        if check:
            assert np.array_equal(rh._engine.get_history(), want)
    e.close()


CREATE = [_dream_everything, _demc_sync, _host_callback, _local_group, _wide_rows]
GROWS = [_history_grows, _running_sums_grow, _outlier_keys_grow, _statistics_scratch_grows, _trace_on_and_off]
SECOND = [_derived_history, _rank_history]


def name(case):
    return case.__name__.strip("_")


def _settled(quiet_s=0.05, limit_s=2.0):
    """the free device memory once it has stopped moving: unchanged over quiet_s of back-to-back readings (no sleeping), within limit_s"""
    t_end = time.monotonic() + limit_s
    last, t_last = _free_device_memory(), time.monotonic()
    while time.monotonic() < t_end and time.monotonic() - t_last < quiet_s:
        now = _free_device_memory()
        if now != last:
            last, t_last = now, time.monotonic()
    return last


def measure(case, limit_s=2.0):
    """-> free device memory after one run of the case minus before it, after one run as a warm-up.  The driver gives the memory of a closed
    sampler back asynchronously, within some tens of milliseconds: the reading before is taken once the warm-up's memory has settled, and
    the reading after is repeated, back to back, until it equals the one before or limit_s have passed -- what is lost never comes back."""
    case()
    gc.collect()
    free0 = _settled()
    case()
    t_end = time.monotonic() + limit_s
    free1 = _free_device_memory()
    while free1 != free0 and time.monotonic() < t_end:
        free1 = _free_device_memory()
    return free1 - free0


if __name__ == "__main__":
    res = {}
    for c in CREATE + GROWS + SECOND:
        res[name(c)] = measure(c)
        print(name(c), res[name(c)], flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f)
