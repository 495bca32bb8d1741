"""bipymc_amd/derived.py: DerivedHistory and HistoryStatistics.derived_history without a GPU.  The engine is a NumPy stand-in put together from
the stand-ins the statistics' own host tests use (one rank each); its derive_history(fn) returns another such engine over fn.python_fn of
every row, in the manner of test_derived_host.FakeDeriveRanks.  Checked: the six statistics see dim = n_out and the parent's n_chains and
return what their own checkers accept on V = fn(history); the object's life (context manager, close, use after close); the refusals (more
than one rank before the engine is touched, something that is no HipFunction, a sampler that has not run); and that the run-time program
still compiles for gfx950 with the fill kernel in it.

Tolerances: those of the imported checkers (test_covariance_host, test_traces_host, test_histograms_host, test_derived_host); quantiles and
values are compared for equality; R-hat / ESS against test_diagnostics_host.reference at 1e-10 / 1e-8 relative, tests/test_gpu_diagnostics.py's."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from bipymc_amd import DerivedHistory, HipFunction  # noqa: E402
from bipymc_amd._history_stats import HistoryStatistics  # noqa: E402
import test_covariance_host as TC  # noqa: E402
import test_histograms_host as TH  # noqa: E402
import test_traces_host as TT  # noqa: E402
from test_derived_host import FakeDeriveRanks, check_summary  # noqa: E402
from test_diagnostics_host import BlockParts, _ar1, reference  # noqa: E402
from test_quantiles_host import StandIn  # noqa: E402

SRC = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[2] / x[1]; out[1] = x[0] * x[0] + x[3]; out[2] = p[0] + p[1] * x[0];
}"""


def _py(X, ll, p):
    with np.errstate(all="ignore"):
        return np.stack([X[:, 2] / X[:, 1], X[:, 0] * X[:, 0] + X[:, 3], p[0] + p[1] * X[:, 0]], axis=1)


FN = HipFunction(SRC, n_out=3, params=[0.25, -3.0], python_fn=_py)
SUM = HipFunction("__device__ void derive(const double* x, int d, double ll, const double* p, double* out) { out[0] = x[0] + x[2]; out[1] = ll; }",
                  n_out=2, python_fn=lambda X, ll, p: np.stack([X[:, 0] + X[:, 2], ll], axis=1))


class FakeEngine(object):
    """one rank's engine over the history H (G, N, d) with log-likelihoods LL (G, N): every call returns the list of one part, which the
    sampler's allgather (the identity) hands on"""

    def __init__(self, H, LL):
        self.H, self.LL = np.asarray(H, dtype=np.float64), np.asarray(LL, dtype=np.float64)
        G, N, d = self.H.shape
        self.n_chains, self.n_local, self.dim = N, N, d
        self.closed = 0
        self.made = []
        cov, hs, tr = TC.FakeRanks(self.H.reshape(-1, d), N, 1), TH.FakeRanks(self.H.reshape(-1, d), N, 1), TT.FakeRanks(self.H, self.LL, 1)
        dg, qs, dv = BlockParts(self.H), StandIn(self.H, 0, N), FakeDeriveRanks(self.H, self.LL, 1)
        self.reduce_moments, self.reduce_cov = cov.reduce_moments, cov.reduce_cov
        self.hist_range, self.hist_marginals, self.hist_pairs = hs.hist_range, hs.hist_marginals, hs.hist_pairs
        self.trace_bins, self.trace_chains = tr.trace_bins, tr.trace_chains
        self.diag_split_moments = lambda a, b: [dg.split(a, b)]
        self.diag_autocov = lambda t0, nl: [dg.autocov(t0, nl)]
        self.quantile_begin = lambda nb: [qs.begin(nb)]
        self.quantile_histogram = lambda a, b, c: [qs.histogram(a, b, c)]
        self.derive = dv.derive

    def history_rows(self):
        return self.H.shape[0]

    def get_history(self):
        return self.H.copy()

    def get_loglike_history(self):
        return self.LL.copy()

    def derive_history(self, fn):
        G, N, d = self.H.shape
        e = FakeEngine(fn(self.H.reshape(-1, d), self.LL.reshape(-1)).reshape(G, N, fn.n_out), self.LL)
        self.made.append(e)
        return e

    def close(self):
        self.closed += 1


class Comm(object):
    def __init__(self, size):
        self.size, self.rank = size, 0


class Sampler(HistoryStatistics):
    def __init__(self, engine, n_chains, comm=None):
        self._engine, self.n_chains = engine, n_chains
        self.asked = []
        if comm is not None:
            self.comm = comm

    def _stats_engine(self, who):
        self.asked.append(who)
        if self._engine is None:
            raise RuntimeError("%s: run_mcmc first" % who)
        return self._engine

    def _stats_allgather(self, obj):
        return obj


def _history(G=40, N=16, d=4, seed=2):
    H = _ar1(G, N, [0.0, 0.5, 0.9, 0.3][:d], seed)
    H[:, :, 1] += 3.0                                   # the denominator of the ratio: away from 0 ...
    H[:, :, 2] += 1e4
    LL = -0.5 * (H[:, :, 0] ** 2) - 10.0
    return H, LL


@pytest.fixture()
def case():
    H, LL = _history()
    G, N, d = H.shape
    s = Sampler(FakeEngine(H, LL), N)
    V = _py(H.reshape(-1, d), LL.reshape(-1), FN.params).reshape(G, N, 3)
    return s, H, LL, V


def test_the_six_statistics_see_the_derived_values_and_the_parents_chains(case):
    s, H, LL, V = case
    G, N, _ = H.shape
    with s.derived_history(FN) as dh:
        assert isinstance(dh, DerivedHistory) and s.asked == ["derived_history"]
        assert dh.n_out == dh.dim == 3 and dh.n_chains == N and dh.history_rows == G
        assert dh._stats_engine("x") is s._engine.made[0] and dh._engine.dim == 3
        mean, std, W = dh.param_est(5)
        assert np.array_equal(W, V.reshape(-1, 3)[5:]) and np.array_equal(mean, W.mean(axis=0)) and np.array_equal(std, W.std(axis=0))
        for n_burn in (0, 3, N * 5 + 1, N * G - 1):
            q = dh.param_est_quantiles(n_burn, q=(0.05, 0.5, 0.95))
            assert q.shape == (3, 3) and np.array_equal(q, np.quantile(V.reshape(-1, 3)[n_burn:], (0.05, 0.5, 0.95), axis=0))
        n_burn = N * 2 + 3
        W = V.reshape(-1, 3)[n_burn:]
        TC.check_against_numpy(dh.param_est_cov(n_burn), W)
        ph = dh.param_est_hist(n_burn, bins=20, pairs="all", bins2d=8)
        assert list(ph.dims) == [0, 1, 2] and len(ph.pairs) == 3
        TH.check_against_numpy(ph, W, bins=20, bins2d=8)
        for every in (1, 7):
            TT.check_against_numpy(dh.param_est_trace(n_burn, every=every, chains=[0, N - 1]), V, LL, n_burn, every, chains=[0, N - 1])
        cd, ref = dh.convergence_diagnostics(n_burn), reference(V, g0=3)
        assert cd.r_hat.shape == (3,)
        np.testing.assert_allclose(cd.r_hat, ref["r_hat"], rtol=1e-10)
        ok = ref["margin"] > 1e-6
        np.testing.assert_allclose(cd.ess[ok], ref["ess"][ok], rtol=1e-8)
        pd = dh.param_est_fn(SUM, n_burn, values=True)               # a function of derived quantities
        want = np.stack([W[:, 0] + W[:, 2], LL.reshape(-1)[n_burn:]], axis=1)
        assert np.array_equal(pd.values, want)
        check_summary(pd, want)
        with dh.derived_history(SUM) as dh2:                           # ... and its history
            assert dh2.n_out == 2 and dh2.n_chains == N
            assert np.array_equal(dh2.param_est(n_burn)[2], want)
    assert [e.closed for e in s._engine.made] == [1] and s._engine.closed == 0


def test_life_of_the_object(case):
    s, H, LL, V = case
    with pytest.raises(KeyError):
        with s.derived_history(FN) as dh:
            raise KeyError("inside")
    eng = s._engine.made[0]
    assert eng.closed == 1 and dh._engine is None
    dh.close()                                                         # a second close is harmless
    dh.close()
    assert eng.closed == 1
    for name, args in (("param_est_quantiles", (0,)), ("convergence_diagnostics", (0,)), ("param_est_cov", (0,)), ("param_est_hist", (0,)),
                       ("param_est_trace", (0,)), ("param_est_fn", (SUM,)), ("param_est", (0,)), ("derived_history", (SUM,))):
        with pytest.raises(RuntimeError, match="^%s: this derived history is closed$" % name):
            getattr(dh, name)(*args)
    dh = s.derived_history(FN)                                         # without `with`: open until closed
    assert s._engine.made[1].closed == 0
    assert dh.param_est_quantiles(0, q=0.5).shape == (3,)
    dh.close()
    assert s._engine.made[1].closed == 1


def test_refusals(case):
    s, H, LL, V = case
    two = Sampler(s._engine, s.n_chains, comm=Comm(2))
    with pytest.raises(NotImplementedError, match="derived_history: a derived history is built on a single rank only .*2 ranks"):
        two.derived_history(FN)
    assert two.asked == [] and s._engine.made == []                    # refused before the engine was asked for
    assert isinstance(Sampler(s._engine, s.n_chains, comm=Comm(1)).derived_history(FN), DerivedHistory)
    for bad in (SRC, _py, None):
        with pytest.raises(TypeError, match="derived_history: fn must be a HipFunction"):
            s.derived_history(bad)
    with pytest.raises(RuntimeError, match="derived_history: run_mcmc first"):
        Sampler(None, 8).derived_history(FN)
    from bipymc_amd.samplers import DeMc
    with pytest.raises(RuntimeError, match="derived_history: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).derived_history(FN)
    from bipymc_amd.engine import HipEngine
    rank = HipEngine.__new__(HipEngine)                                # the engine's own refusal: nothing is installed or created
    rank._h, rank.world_size = None, 2
    with pytest.raises(NotImplementedError, match=r"derive_history: a derived history is built on a single rank only \(world_size = 2\)"):
        rank.derive_history(FN)
    from bipymc_amd import DeMcMpi, DreamMpi
    assert all(hasattr(c, "derived_history") for c in (DeMc, DeMcMpi, DreamMpi))


def test_the_run_time_program_compiles_with_the_fill_kernel_and_keeps_the_callers_line_numbers():
    from bipymc_amd import _lib as L
    assert FN.check() and SUM.check("gfx950")
    assert hasattr(L.load(), "bpm_derive_history") and "bpm_derive_history" in L.SIGNATURES
    rows = open(os.path.join(os.path.dirname(HERE), "bipymc_amd", "csrc", "derive_rows.h")).read()
    assert rows.count("__global__") == 2 and "bpm_derive_fill(" in rows and "bpm_derive_rows(" in rows
    assert rows.count("v[u] = src[") == 1                              # one staging loop, used by both kernels
    broken = "\n\n__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {\n    out[0] = x[0]\n}"
    with pytest.raises(ValueError, match=r"does not compile(.|\n)*derive\.hip:4:\d+: error: expected"):
        HipFunction(broken, n_out=1).check()
    # no GPU needed to be refused by name: null handles never reach a device call
    lib = L.load()
    assert lib.bpm_derive_history(None, None) != 0 and b"bpm_derive_history: null handle" in lib.bpm_last_error()
