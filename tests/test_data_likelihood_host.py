"""The per-datum form of HipLikelihood without a GPU: argument validation, the compile-only check of its run-time program (hiprtc builds it for gfx950
on any machine), the test likelihood's exact reference against its own bound (tests/_data_likelihood_cases.py), and a sampler class running a
data= likelihood on its python_fn through the CPU test engine."""
import math

import numpy as np
import pytest

import _data_likelihood_cases as DC

P = [0.75, 0.125]


def _ll(K=1, w=3, n=10, **kw):
    from bipymc_amd import HipLikelihood
    data = DC.make_data(n, w)
    return HipLikelihood(DC.hip_source(K, w), params=P, data=data, terms=K, python_fn=DC.python_fn(K, data, P), **kw)


def test_data_arguments_are_validated():
    from bipymc_amd import HipLikelihood
    src = DC.hip_source(1, 3)
    ll = HipLikelihood(src, params=P, data=np.zeros((5, 3)), terms=1)
    assert ll.data.shape == (5, 3) and ll.data.dtype == np.float64 and ll.data.flags["C_CONTIGUOUS"]
    assert ll.source.startswith("#define BPM_LN_LIKE_DATA 1\n#define BPM_LN_LIKE_DATA_W 3\n") and "BPM_LN_LIKE_TERMS" not in ll.source
    one = HipLikelihood(src, data=np.zeros(7), terms=2)                      # 1-D: w = 1
    assert one.data.shape == (7, 1) and "#define BPM_LN_LIKE_DATA 2\n#define BPM_LN_LIKE_DATA_W 1\n" in one.source
    strided = HipLikelihood(src, data=np.arange(24.0).reshape(4, 6)[:, ::2], terms=1)
    assert strided.data.flags["C_CONTIGUOUS"] and np.array_equal(strided.data[1], [6.0, 8.0, 10.0])
    with pytest.raises(ValueError, match="terms"):
        HipLikelihood(src, data=np.zeros((5, 3)))                            # data without terms
    with pytest.raises(ValueError, match="terms"):
        HipLikelihood(src, data=np.zeros((5, 3)), terms=9)
    with pytest.raises(ValueError, match="float64"):
        HipLikelihood(src, data=np.zeros((5, 3), dtype=np.float32), terms=1)
    with pytest.raises(ValueError, match="float64"):
        HipLikelihood(src, data=np.zeros((5, 3), dtype=np.int64), terms=1)
    with pytest.raises(ValueError, match="shape"):
        HipLikelihood(src, data=np.zeros((5, 3, 2)), terms=1)
    with pytest.raises(ValueError, match="n_data"):
        HipLikelihood(src, data=np.zeros((0, 3)), terms=1)
    with pytest.raises(ValueError, match="w <= 64"):
        HipLikelihood(src, data=np.zeros((5, 65)), terms=1)
    with pytest.raises(ValueError, match="w <= 64"):
        HipLikelihood(src, data=np.zeros((5, 0)), terms=1)
    assert HipLikelihood(src, data=np.zeros((2, 64)), terms=8).data.shape == (2, 64)
    # the other forms are what they were
    assert HipLikelihood("x", terms=2).source == "#define BPM_LN_LIKE_TERMS 2\nx" and HipLikelihood("x").source == "x" and HipLikelihood("x").data is None


@pytest.mark.parametrize("K", [1, 8])
def test_check_compiles_the_per_datum_program_without_a_gpu(K):
    assert _ll(K=K, w=3).check() is True
    assert _ll(K=K, w=1).check() is True


def test_check_names_the_signature_when_ln_like_datum_is_missing():
    from bipymc_amd import HipLikelihood
    plain = "__device__ double ln_like(const double* x, int d, const double* p) { return -0.5 * x[0] * x[0]; }"
    with pytest.raises(ValueError) as e:
        HipLikelihood(plain, data=np.zeros((4, 2)), terms=1).check()
    msg = str(e.value)
    assert "void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc)" in msg
    assert "double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p)" in msg
    assert "ln_like_datum" in msg.split("):\n", 1)[1]                        # ... and the compiler's log says what is missing


def test_the_plain_and_the_terms_form_still_compile():
    from bipymc_amd import HipLikelihood
    assert HipLikelihood(DC.plain_source(2, 5), params=np.zeros(12)).check()
    assert HipLikelihood("__device__ void ln_like_terms(double xj, int j, int d, const double* p, double* acc) { acc[0] += xj * xj; }\n"
                         "__device__ double ln_like_finish(const double* acc, int d, const double* p) { return -0.5 * acc[0]; }", terms=1).check()


@pytest.mark.parametrize("w", [1, 3])
def test_exact_reference_agrees_with_fsum_within_its_own_bound(w):
    """the moment form of the exact value is the definition (term by term in Fractions, bit for bit), and math.fsum over the NumPy terms -- the
    correctly rounded sum of ROUNDED terms -- and python_fn are within the bound of it"""
    C = 4096
    sizes = [1, 63, 65, 700, C + 1]
    data = DC.make_data(max(sizes), w)
    mom = DC.Moments(data, sizes)
    for d in (3, 5):
        X = DC.make_rows(3, d, w)
        for n in sizes:
            t, y = DC.split(data[:n])
            for K in (1, 2):
                for x in X:
                    ref = DC.exact_value(x, mom.at[n], P, K)
                    if n <= 700:
                        assert ref == DC.exact_value_termwise(x, data[:n], P, K)
                    r = y - (x[0] + x[1] * t + x[2] * (t * t))
                    v = -0.5 * math.fsum(r * r * P[0]) + (P[1] * math.fsum(r) if K >= 2 else 0.0) - 0.5 * (x[-1] * x[-1])
                    b = DC.error_bound(x, data[:n], P, K, C)
                    assert 0.0 < b < 1e-9 * max(1.0, abs(ref))               # (a bound that bounds nothing would pass everything)
                    assert abs(v - ref) <= b, (w, d, n, K, v - ref, b)
                    assert abs(DC.python_fn(K, data[:n], P)(x) - ref) <= b


def test_a_sampler_runs_a_data_likelihood_on_its_python_fn(oracle_engine, monkeypatch):
    """Through the CPU test engine (tests/_oracle_engine.py: the oracle sampler behind the engine's interface, its ll_fn the likelihood's python_fn)
    DreamMpi runs a HipLikelihood with data: the class hands the engine source, params AND data, and every ln-like of the run is python_fn's.
    (The test engine steps only by step(); the two methods added here stand for the HIP engine's, which compile the source.)"""
    import _oracle_engine
    import bipymc_amd.demc as D
    from bipymc_amd import DreamMpi
    ll = _ll(K=2, w=3, n=200)
    theta_0 = np.array([0.5, 2.0, -1.5])
    assert ll(theta_0) == DC.python_fn(2, ll.data, P)(theta_0)
    seen = []

    class Engine(_oracle_engine.OracleEngine):
        def set_device_likelihood(self, source, params=(), data=None):
            seen.append((source, np.asarray(params), data))

        def refresh_device_loglike(self):
            self.s.ll = self.s._ll(self.s.X)
            self.s.ll_history[-1] = self.s.ll[self.lo:self.lo + self.n_local].copy()

    monkeypatch.setattr(D, "_engine_factory", lambda **kw: Engine(ll_fn=ll.python_fn, **kw))
    s = DreamMpi(ll, theta_0, n_chains=8, seed=3, burnin_gen=4, n_cr_gen=2)
    assert len(seen) == 1 and seen[0][0] == ll.source and np.array_equal(seen[0][1], P) and seen[0][2] is ll.data
    s.run_mcmc(8 * 12)
    mean, sd, chain = s.param_est(n_burn=8)
    assert chain.shape[1] == 3 and np.all(np.isfinite(mean)) and np.all(sd > 0)
    lls = np.array([ll(x) for x in s._engine.get_state()])
    np.testing.assert_array_equal(s._engine.get_loglike(), lls)


def test_more_than_one_rank_is_refused_before_anything_is_created(oracle_engine):
    from bipymc_amd import DeMcMpi, DreamMpi

    class TwoRanks(object):
        rank, size = 0, 2

        def bcast(self, obj, root=0):
            raise AssertionError("the constructor went on to talk to the other rank")
        allgather = Barrier = bcast

    for cls in (DreamMpi, DeMcMpi):
        with pytest.raises(NotImplementedError, match="2 ranks"):
            cls(_ll(), np.zeros(3), n_chains=8, mpi_comm=TwoRanks(), seed=1)


def test_a_callable_that_keeps_its_data_in_an_attribute_is_no_data_likelihood(monkeypatch):
    """Only a HipLikelihood with data is refused on several ranks: an ordinary host callable written as a class that keeps its data set in `self.data` is
    constructed with two ranks as ever, and its start states are evaluated by calling it."""
    import bipymc_amd.demc as D
    from bipymc_amd import DeMcMpi, DreamMpi

    class Fit(object):
        def __init__(self):
            self.data = np.arange(6.0)

        def __call__(self, theta):
            return -0.5 * float(np.sum((self.data[:3] - theta) ** 2))

    class TwoRanks(object):
        rank, size = 1, 2

        def bcast(self, obj, root=0):
            return obj if obj is not None else 17

        def allgather(self, obj):
            return [obj, obj]

        def Barrier(self):
            pass

    class Engine(object):
        def __init__(self, n_chains, dim, world_size, **kw):
            self.n_local, self.X, self.ll = n_chains // world_size, np.ones((n_chains, dim)), None

        def init_chains(self, theta_0, varepsilon):
            pass

        def get_state(self):
            return self.X

        def set_loglike(self, ll):
            self.ll = np.asarray(ll)

    monkeypatch.setattr(D, "_engine_factory", lambda **kw: Engine(**kw))
    for cls in (DreamMpi, DeMcMpi):
        s = cls(Fit(), np.zeros(3), n_chains=8, mpi_comm=TwoRanks(), seed=1)
        assert s._hip_likelihood is None and s._engine.ll.shape == (4,) and np.all(s._engine.ll == -0.5 * (1.0 + 0.0 + 1.0))


def test_the_form_is_read_from_the_define_line_itself():
    """bpm_check_device_likelihood routes a source by its `#define BPM_LN_LIKE_DATA K` line, blanks as the preprocessor allows them; the name in a comment,
    or BPM_LN_LIKE_DATA_W alone, does not make a plain source a per-datum one"""
    from bipymc_amd import HipLikelihood
    body = DC.hip_source(1, 3)
    for head in ("#define BPM_LN_LIKE_DATA 1\n#define BPM_LN_LIKE_DATA_W 3\n", "  #  define\tBPM_LN_LIKE_DATA   1\r\n#define BPM_LN_LIKE_DATA_W\t3\n"):
        assert HipLikelihood(head + body).check()                  # (no ln_like in it: only the per-datum header compiles around it)
    plain = "__device__ double ln_like(const double* x, int d, const double* p) { return -0.5 * x[0] * x[0]; }\n"
    for note in ("// not the form with #define BPM_LN_LIKE_DATA 2\n", "/* #define BPM_LN_LIKE_DATA 2 */\n", "#define BPM_LN_LIKE_DATA_W 3\n", "#define BPM_LN_LIKE_DATA2 1\n"):
        assert HipLikelihood(note + plain).check()
