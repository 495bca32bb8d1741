"""The per-datum form of HipLikelihood on the device (bipymc_amd/csrc/user_eval_data.h; bpm_set_device_likelihood_data, bpm_eval_device_likelihood):
values against the exact reference within the derived bound, the bit-for-bit invariance of a row's value, whole runs against the CPU oracle and against
the same likelihood in the plain form, non-finite values, ownership, and the sampler classes.  The likelihood, its exact value and the bound:
tests/_data_likelihood_cases.py -- no tolerance here was tuned on a GPU."""
import numpy as np
import pytest

import _data_likelihood_cases as DC
from oracle import sampler_ref as R

pytestmark = pytest.mark.gpu

P = [0.75, 0.125]
WHY = "summed over its data by kernels of its own"


def _engine(**kw):
    from bipymc_amd.engine import HipEngine
    return HipEngine(**kw)


def _chunk():
    from bipymc_amd.engine import HipEngine
    return HipEngine.data_likelihood_chunk()


_cache = {}


def _data(w):
    """the data of every case with this w (a case takes the first n_data rows), the sizes of the value test, and the exact moments at those sizes and
    at the sizes of the runs against the oracle (200, one chunk + 100): computed once"""
    if w not in _cache:
        C = _chunk()
        sizes = [1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 17]
        data = DC.make_data(max(sizes), w)
        _cache[w] = (data, sizes, DC.Moments(data, sizes + [200, C + 100]))
    return _cache[w]


def _host_engine(d, N=16, algo=R.ALGO_DREAM, seed=78, **kw):
    return _engine(algo=algo, n_chains=N, dim=d, target_id=R.TARGET_HOST, target_params=None, seed=seed, **kw)


# ------------------------------------------------------------------ 1. values
def test_the_chunk_is_a_multiple_of_the_wavefront():
    C = _chunk()
    assert C >= 64 and C % 64 == 0


@pytest.mark.parametrize("d", [3, 5, 640])
@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("w", [1, 3])
def test_values_against_the_exact_reference(w, K, d):
    """eval_device_likelihood on 8 rows at every n_data where the kernels take another way (one lane, a partial and a full first round of the lanes,
    one past it; one datum short of a chunk, a chunk, one past it: the fold; two chunks and a ragged third) against the correctly rounded exact value,
    within the derived bound.  K = 8: ln_like_total returns NaN unless the six unused sums are still exactly zero.  d = 640: rows too wide for the
    staged copy, read where they lie at their padded stride; the total's -0.5 x[d-1]^2 shows a row that was staged or strided wrongly."""
    data, sizes, mom = _data(w)
    C = _chunk()
    X = DC.make_rows(8, d, w)
    eng = _host_engine(d)
    try:
        for n in sizes:
            eng.set_device_likelihood("#define BPM_LN_LIKE_DATA %d\n#define BPM_LN_LIKE_DATA_W %d\n" % (K, w) + DC.hip_source(K, w), P, data=data[:n])
            assert eng.device_likelihood_info()[0] is False and WHY in eng.device_likelihood_info()[1]
            got = eng.eval_device_likelihood(X)
            for x, v in zip(X, got):
                ref = DC.exact_value(x, mom.at[n], P, K)
                b = DC.error_bound(x, data[:n], P, K, C)
                print("w %d K %d d %d n_data %d: error %.3e bound %.3e" % (w, K, d, n, v - ref, b))
                assert abs(v - ref) <= b, (w, K, d, n, v, ref, b)
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. invariance, bit for bit
@pytest.mark.parametrize("d", [5, 640])
def test_a_rows_value_depends_on_nothing_but_the_row(d):
    """The same x alone among 4 rows, as the first and as the last of 257 rows (more than one batch of the chunk-sum scratch), and as the state of
    different chains after set_state + refresh_device_loglike: identical bits, with one chunk (n_data = 65) and with three (2 C + 17).  And what
    installation leaves in get_loglike() is eval_device_likelihood of the states."""
    C = _chunk()
    w, K, N = 3, 2, 16
    data = _data(w)[0]
    others = DC.make_rows(257, d, w, seed=9)
    x = DC.make_rows(1, d, w, seed=3)[0]
    eng = _host_engine(d, N=N)
    try:
        X0 = DC.make_rows(N, d, w, seed=4)
        eng.set_state(X0)
        for n in (65, 2 * C + 17):
            eng.set_device_likelihood("#define BPM_LN_LIKE_DATA %d\n#define BPM_LN_LIKE_DATA_W %d\n" % (K, w) + DC.hip_source(K, w), P, data=data[:n])
            assert np.array_equal(eng.get_loglike(), eng.eval_device_likelihood(eng.get_state()))
            few = others[:4].copy()
            few[2] = x
            v = eng.eval_device_likelihood(few)[2]
            assert np.isfinite(v) and abs(v - DC.exact_value(x, _data(w)[2].at[n], P, K)) <= DC.error_bound(x, data[:n], P, K, C)
            many = others.copy()
            many[0] = x
            many[256] = x
            got = eng.eval_device_likelihood(many)
            assert got[0] == v and got[256] == v
            assert np.array_equal(got[1:256], eng.eval_device_likelihood(others[1:256]))      # ... and so does every other row's
            for slot in (0, 7, N - 1):
                Xs = X0.copy()
                Xs[slot] = x
                eng.set_state(Xs)
                eng.refresh_device_loglike()
                assert eng.get_loglike()[slot] == v, (n, slot)
            eng.set_state(X0)
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. against the oracle
def _start(N, d, w=3):
    X0 = np.random.RandomState(5).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0)
    X0[:, :3] = DC.make_rows(N, 3, w, seed=6)
    return X0


def _check_ll(eng, mom, data, K, C):
    """the engine's ln-likes are the EXACT likelihood of its own states, correctly rounded, within the derived bound (mom: the exact moments of `data`)"""
    X, ll = eng.get_state(), eng.get_loglike()
    for x, v in zip(X, ll):
        ref = DC.exact_value(x, mom, P, K)
        assert abs(v - ref) <= DC.error_bound(x, data, P, K, C), (v, ref)


@pytest.mark.parametrize("n_extra", [None, 100])
@pytest.mark.parametrize("algo,d,N,kw", [
    (R.ALGO_DREAM, 3, 16, dict(burnin_gen=5, n_cr_gen=2)),
    (R.ALGO_DEMC, 3, 24, dict(p_snooker=0.3)),
    (R.ALGO_DEMC_SYNC, 3, 10, dict()),
    (R.ALGO_DREAM, 600, 12, dict(burnin_gen=5, n_cr_gen=1)),
])
def test_data_likelihood_against_oracle(algo, d, N, kw, n_extra):
    """The pattern of test_hip_source_likelihood_against_oracle: the sampler driven by bpm_step with the per-datum likelihood between its proposal and commit
    kernels against OracleSampler(ll_fn = python_fn) -- accept counts equal, state and whole history to 1e-11 / 1e-13, CR statistics to 1e-9; several step
    calls, then a state rewritten from the host.  The ln-likes: within the derived bound of the exact value at the engine's own states (the oracle's states
    may differ from the engine's in the last bits, which an evaluation bound does not cover), at n_data = 200 and at one chunk + 100 (the fold)."""
    C = _chunk()
    n = 200 if n_extra is None else C + n_extra
    w, K = 3, 2
    data, mom = _data(w)[0][:n], _data(w)[2].at[n]
    py_ll = DC.python_fn(K, data, P)
    eng = _host_engine(d, N=N, algo=algo, **kw)
    ora = R.OracleSampler(algo, N, d, R.TARGET_HOST, None, 78, ll_fn=py_ll, **kw)
    try:
        X0 = _start(N, d)
        eng.set_state(X0)
        eng.set_device_likelihood("#define BPM_LN_LIKE_DATA %d\n#define BPM_LN_LIKE_DATA_W %d\n" % (K, w) + DC.hip_source(K, w), P, data=data)
        assert eng.device_likelihood_info()[0] is False
        _check_ll(eng, mom, data, K, C)
        ora.set_state(X0)
        eng.begin_run()
        g = 0
        for k in (1, 4, 2):
            eng.step(k)
            for _ in range(k):
                ora._generation(g, 0.5, True, 1e-12 if algo == R.ALGO_DREAM else 1e-15, 1e-2, None)
                g += 1
            np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-11, atol=1e-13)
            _check_ll(eng, mom, data, K, C)
        st = eng.stats()
        assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected
        assert st["local_n_accepted"] > 0
        if algo == R.ALGO_DREAM:
            np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)
            np.testing.assert_allclose(st["n_cr_updates"], ora.cr.n_cr_updates, rtol=0)
        np.testing.assert_allclose(eng.get_history(), ora.history_array(), rtol=1e-11, atol=1e-13)
        X1 = eng.get_state() + 0.125 * np.concatenate([DC.x_scale(w), np.ones(d - 3)])
        eng.set_state(X1)
        eng.refresh_device_loglike()
        _check_ll(eng, mom, data, K, C)
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. same answers as the plain form
def _plain(K, data):
    return DC.plain_source(K, len(data)), np.concatenate([P, data[:, :2].reshape(-1)])


@pytest.mark.parametrize("fused", [False, True])
def test_same_run_as_the_plain_form(fused, monkeypatch):
    """The same likelihood as plain ln_like, its data inside params -- three kernels (BPM_USER_FUSED=0) and inside the update kernel -- gives the same run:
    accept counts equal, state and history at the oracle test's tolerances after 12 generations (the two forms add the terms in different orders)."""
    w, K, N, d, n = 3, 2, 16, 3, 200
    data = _data(w)[0][:n]
    runs = []
    for form in ("data", "plain"):
        eng = _host_engine(d, N=N, burnin_gen=6, n_cr_gen=2)
        try:
            eng.set_state(_start(N, d))
            if form == "data":
                eng.set_device_likelihood("#define BPM_LN_LIKE_DATA %d\n#define BPM_LN_LIKE_DATA_W %d\n" % (K, w) + DC.hip_source(K, w), P, data=data)
            else:
                monkeypatch.setenv("BPM_USER_FUSED", "1" if fused else "0")
                eng.set_device_likelihood(*_plain(K, data))
            assert eng.device_likelihood_info()[0] == (form == "plain" and fused)
            eng.begin_run()
            eng.step(12)
            st = eng.stats()
            runs.append((st["local_n_accepted"], st["local_n_rejected"], eng.get_state(), eng.get_history(), eng.get_loglike()))
        finally:
            eng.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and 0 < a[0] < 12 * N
    np.testing.assert_allclose(a[2], b[2], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(a[3], b[3], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(a[4], b[4], rtol=1e-11, atol=1e-12)


# ------------------------------------------------------------------ 5. non-finite
PRIOR_SRC = """
__device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc) {
    const double r = y[1] - (x[0] + x[1] * y[0] + x[2] * (y[0] * y[0]));
    acc[0] += r * r * p[0];
}
__device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p) {
    if (x[0] < p[1]) return -INFINITY;                              // a prior: x_0 above a bound
    return -0.5 * acc[0];
}"""
NAN_SRC = """
__device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc) {
    const double r = y[1] - (x[0] + x[1] * y[0] + x[2] * (y[0] * y[0]));
    acc[0] += r * r * p[0] * sqrt(p[1] - x[0]);                     // NaN for x_0 > p_1
}
__device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p) { return -0.5 * acc[0]; }"""


def test_rows_outside_the_prior_are_never_accepted():
    """ln_like_total returns -INFINITY below a bound on x_0 that lies just under the start states: such proposals get -inf (eval_device_likelihood says so)
    and no chain ever moves there -- the run is the oracle's with the same function in NumPy, accept for accept."""
    w, N, d, n = 3, 24, 3, 300
    data = _data(w)[0][:n]
    t, y = DC.split(data)
    X0 = _start(N, d)
    bound = float(X0[:, 0].min()) - 0.01

    def py_ll(th):
        th = np.asarray(th, dtype=np.float64).reshape(-1)
        if th[0] < bound:
            return -np.inf
        r = y - (th[0] + th[1] * t + th[2] * (t * t))
        return float(-0.5 * np.sum(r * r * P[0]))

    eng = _host_engine(d, N=N, algo=R.ALGO_DEMC, p_snooker=0.1)
    ora = R.OracleSampler(R.ALGO_DEMC, N, d, R.TARGET_HOST, None, 78, ll_fn=py_ll, p_snooker=0.1)
    try:
        eng.set_state(X0)
        eng.set_device_likelihood("#define BPM_LN_LIKE_DATA 1\n#define BPM_LN_LIKE_DATA_W 3\n" + PRIOR_SRC, [P[0], bound], data=data)
        out = X0[:4].copy()
        out[:, 0] = bound - np.array([1e-9, 0.1, 1.0, 1e6])
        assert np.all(eng.eval_device_likelihood(out) == -np.inf) and np.all(np.isfinite(eng.eval_device_likelihood(X0)))
        ora.set_state(X0)
        eng.begin_run()
        eng.step(15)
        for g in range(15):
            ora._generation(g, 0.5, True, 1e-15, 1e-2, None)
        H = eng.get_history()
        assert H[:, :, 0].min() >= bound
        st = eng.stats()
        assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected and st["n_nan_alpha"] == 0
        np.testing.assert_allclose(H, ora.history_array(), rtol=1e-11, atol=1e-13)
        assert np.all(np.isfinite(eng.get_loglike()))
    finally:
        eng.close()


def test_a_nan_from_the_datum_function_raises_through_the_sampler_class():
    """exactly as with a callable (samplers.py:336): a NaN ln-like among the proposals makes run_mcmc raise ValueError("probabilities contain NaN")"""
    from bipymc_amd import DreamMpi, HipLikelihood
    w, n = 3, 150
    data = _data(w)[0][:n]
    theta_0 = np.array([0.5, 2.0, -1.5])
    ll = HipLikelihood(NAN_SRC, params=[P[0], 0.5 + 1e-4], data=data, terms=1)      # (the chains start 1e-4, three of their standard deviations, below the edge and spread over it)
    s = DreamMpi(ll, theta_0, varepsilon=1e-9, n_chains=16, seed=4, burnin_gen=10, n_cr_gen=2)
    assert np.all(np.isfinite(s._engine.get_loglike()))
    with pytest.raises(ValueError, match="probabilities contain NaN"):
        s.run_mcmc(16 * 60)


# ------------------------------------------------------------------ 6. ownership
def test_installing_replacing_and_closing():
    """per-datum -> plain -> per-datum with another n_data -> close, device_likelihood_info right at every step; a source that does not compile in the
    middle leaves the installed likelihood working (same bits); no likelihood installed: bpm_eval_device_likelihood is an error that says so."""
    C = _chunk()
    w, K, N, d = 3, 2, 16, 3
    data = _data(w)[0]
    head = "#define BPM_LN_LIKE_DATA %d\n#define BPM_LN_LIKE_DATA_W %d\n" % (K, w)
    X = DC.make_rows(5, d, w)
    eng = _host_engine(d, N=N)
    try:
        eng.set_state(_start(N, d))
        with pytest.raises(Exception, match="no device likelihood installed"):
            eng.eval_device_likelihood(X)
        with pytest.raises(Exception, match="no device likelihood installed"):
            eng.device_likelihood_info()
        eng.set_device_likelihood(head + DC.hip_source(K, w), P, data=data[:65])
        assert eng.device_likelihood_info()[0] is False and WHY in eng.device_likelihood_info()[1]
        v65 = eng.eval_device_likelihood(X)
        with pytest.raises(Exception, match="does not compile"):
            eng.set_device_likelihood(head + "__device__ double ln_like_total(const double* x) { return x[0] }", P, data=data[:65])
        with pytest.raises(Exception, match="bpm_set_device_likelihood_data"):
            eng.set_device_likelihood(head + DC.hip_source(K, w), P)                       # a per-datum source without its data
        with pytest.raises(Exception, match="BPM_LN_LIKE_DATA"):
            eng.set_device_likelihood(DC.plain_source(K, 65), _plain(K, data[:65])[1], data=data[:65])
        with pytest.raises(Exception, match="values per datum"):
            eng.set_device_likelihood(head + DC.hip_source(K, w), P, data=data[:65, :2])   # written for w = 3, given w = 2
        assert eng.device_likelihood_info()[0] is False and np.array_equal(eng.eval_device_likelihood(X), v65)
        eng.begin_run()
        eng.step(2)
        eng.set_device_likelihood(*_plain(K, data[:65]))
        assert eng.device_likelihood_info()[0] is True, eng.device_likelihood_info()[1]
        np.testing.assert_allclose(eng.eval_device_likelihood(X), v65, rtol=1e-12)
        eng.step(2)
        n2 = C + 100
        eng.set_device_likelihood(head + DC.hip_source(K, w), P, data=data[:n2])
        assert eng.device_likelihood_info()[0] is False and WHY in eng.device_likelihood_info()[1]
        for x, v in zip(X, eng.eval_device_likelihood(X)):
            assert abs(v - DC.exact_value(x, _data(w)[2].at[n2], P, K)) <= DC.error_bound(x, data[:n2], P, K, C)
        eng.step(2)
        assert np.array_equal(eng.get_loglike(), eng.eval_device_likelihood(eng.get_state()))
    finally:
        eng.close()


TERMS_SRC = """
__device__ void ln_like_terms(double xj, int j, int d, const double* p, double* acc) { const double z = (xj - p[j]) * p[d + j]; acc[0] += z * z; acc[1] += z; }
__device__ double ln_like_finish(const double* acc, int d, const double* p) { return -0.5 * acc[0] + 0.25 * acc[1]; }
"""


@pytest.mark.parametrize("form", ["plain", "terms"])
def test_eval_device_likelihood_serves_the_other_forms_too(form, monkeypatch):
    """The plain and the per-coordinate form through bpm_eval_device_likelihood: their kernel of their own, bpm_user_eval (a thread per row), whether the
    likelihood is installed fused or not.  Installed unfused, the cached ln-likes come from that same kernel: equal bits; installed fused, the entry
    returns the unfused installation's values bit for bit; and the values are the formula's (NumPy, 1e-12: another order of the additions)."""
    w, K, d, N = 3, 2, 5, 16
    data = _data(w)[0][:65]
    X = DC.make_rows(70, d, w)
    if form == "plain":
        src, params = _plain(K, data)
        py = DC.python_fn(K, data, P)
    else:
        mu, isd = np.arange(d) * 0.25, 1.0 / (1.0 + 0.5 * np.arange(d))
        src, params = "#define BPM_LN_LIKE_TERMS 2\n" + TERMS_SRC, np.concatenate([mu, isd])

        def py(x):
            z = (x - mu) * isd
            return -0.5 * np.sum(z * z) + 0.25 * np.sum(z)
    got = {}
    for fused in (False, True):
        monkeypatch.setenv("BPM_USER_FUSED", "1" if fused else "0")
        eng = _host_engine(d, N=N)
        try:
            eng.set_state(X[:N])
            eng.set_device_likelihood(src, params)
            assert eng.device_likelihood_info()[0] is fused, eng.device_likelihood_info()[1]
            got[fused] = eng.eval_device_likelihood(X)
            if not fused:
                assert np.array_equal(eng.get_loglike(), got[fused][:N])
        finally:
            eng.close()
    assert np.array_equal(got[False], got[True])
    np.testing.assert_allclose(got[True], [py(x) for x in X], rtol=1e-12)


# ------------------------------------------------------------------ 7. through the classes
def test_through_the_sampler_classes():
    """DreamMpi, DeMcMpi and DeMc with a data= likelihood, 16 chains, 30 generations: the run of the plain form (param_est's chain at the tolerances of the
    plain-form test, accept counts equal), posterior_summary() works; more than one rank: NotImplementedError before anything is created."""
    from bipymc_amd import DeMcMpi, DreamMpi, HipLikelihood
    from bipymc_amd.samplers import DeMc
    w, K, N, n = 3, 2, 16, 1000
    data = _data(w)[0][:n]
    theta_0 = np.array([0.5, 2.0, -1.5])
    per_datum = HipLikelihood(DC.hip_source(K, w), params=P, data=data, terms=K, python_fn=DC.python_fn(K, data, P))
    src, params = _plain(K, data)
    plain = HipLikelihood(src, params=params)
    for cls, kw in ((DreamMpi, dict(n_cr_gen=5, burnin_gen=10)), (DeMcMpi, dict(p_snooker=0.1))):
        a = cls(per_datum, theta_0, varepsilon=1e-4, n_chains=N, seed=21, **kw)
        b = cls(plain, theta_0, varepsilon=1e-4, n_chains=N, seed=21, **kw)
        assert a._hip_likelihood is per_datum and a._engine.device_likelihood_info()[0] is False and b._engine.device_likelihood_info()[0] is True
        a.run_mcmc(N * 31)
        b.run_mcmc(N * 31)
        assert a.local_n_accepted == b.local_n_accepted and a.local_n_rejected == b.local_n_rejected and a.local_n_accepted > 0
        for u, v in zip(a.param_est(0), b.param_est(0)):
            np.testing.assert_allclose(u, v, rtol=1e-11, atol=1e-13)
        assert a.param_est(0)[2].shape[1] == 3 and a.posterior_summary() is not None
    runs = []
    for fn in (per_datum, plain):
        sd = DeMc(fn, n_chains=N, seed=9)
        sd.run_mcmc(N * 31, theta_0, varepsilon=1e-4)
        runs.append((sd.n_accepted, sd.param_est(0)))
        assert sd.posterior_summary() is not None
    assert runs[0][0] == runs[1][0] and runs[0][0] > 1
    for u, v in zip(runs[0][1], runs[1][1]):
        np.testing.assert_allclose(u, v, rtol=1e-11, atol=1e-13)

    class TwoRanks(object):
        rank, size = 0, 2

    for cls in (DreamMpi, DeMcMpi):
        with pytest.raises(NotImplementedError, match="2 ranks"):
            cls(per_datum, theta_0, n_chains=N, mpi_comm=TwoRanks(), seed=1)
