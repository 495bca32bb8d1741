"""bipymc_amd/derived.py without a GPU: HipFunction's compile-only check (hiprtc builds the wrapper of bipymc_amd/csrc/derived.h around the
caller's function for gfx950), and derived.compute driven by a NumPy stand-in for the device call -- python_fn over each fake rank's rows of
param_est's window, handed over as traces.h's records (shift = the rank's first finite value, blocked partial sums in another order than
NumPy's) -- on 1, 2 and 4 emulated ranks with a partial first generation.

Tolerance: mean and sd lie within trace_bound (tests/test_traces_host.py, derived there for any summation order) of a np.longdouble
evaluation of the values; min, max, n_nan, n and the values themselves are compared for equality."""
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from bipymc_amd import HipFunction, PosteriorDerived  # noqa: E402
from bipymc_amd import derived as DV  # noqa: E402
from test_traces_host import FakeRanks, trace_bound  # noqa: E402

LINE = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[2] / x[1];
    for (int k = 0; k < 64; ++k) out[1 + k] = x[0] + x[1] * p[k];
}"""


def check_summary(pd, V, what=""):
    """pd: the PosteriorDerived of the values V (rows, n_out): every field against NumPy on V (the module docstring's tolerances)"""
    V = np.asarray(V, dtype=np.float64)
    n, m = V.shape
    assert pd.n == n and pd.mean.shape == pd.sd.shape == pd.min.shape == pd.max.shape == pd.n_nan.shape == (m,), what
    assert pd.n_nan.dtype == np.int64 and np.array_equal(pd.n_nan, np.isnan(V).sum(axis=0)), what
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(pd.min, np.nanmin(V, axis=0), equal_nan=True), what
        assert np.array_equal(pd.max, np.nanmax(V, axis=0), equal_nan=True), what
        want_m, want_s = np.mean(V, axis=0), np.std(V, axis=0)
    fin = np.isfinite(V).all(axis=0)
    assert np.array_equal(pd.mean[~fin], want_m[~fin], equal_nan=True), what
    assert np.all(np.isnan(pd.sd[~fin])) and np.all(np.isnan(want_s[~fin])), what
    for k in np.nonzero(fin)[0]:
        v = V[:, k].astype(np.longdouble)
        mu = v.sum() / n
        var = ((v - mu) ** 2).sum() / n
        bm, bv = trace_bound(n, float(np.abs(V[:, k]).max()), float(np.abs(v - mu).max()))
        em, ev = float(abs(np.longdouble(pd.mean[k]) - mu)), float(abs(np.longdouble(pd.sd[k]) ** 2 - var))
        assert em <= bm, (what, k, em, bm)
        assert ev <= bv, (what, k, ev, bv)


class FakeDeriveRanks(object):
    """bpm_derive of R ranks over the history H (G, N, d) with log-likelihoods LL (G, N): rank r holds the chains [r N / R, (r + 1) N / R)
    and evaluates fn.python_fn on its rows of param_est's window (rows >= n_burn of the super chain, a partial first generation by chain
    index)"""

    def __init__(self, H, LL, R):
        self.H, self.LL, self.R = np.asarray(H, dtype=np.float64), np.asarray(LL, dtype=np.float64), R
        self.G, self.N, self.d = self.H.shape
        self.n_local = self.N // R

    def derive(self, fn, n_burn, values):
        out = []
        for r in range(self.R):
            lo = r * self.n_local
            g0 = n_burn // self.N
            first = min(max(n_burn % self.N - lo, 0), self.n_local)
            X = self.H[g0:, lo:lo + self.n_local].reshape(-1, self.d)[first:]
            ll = self.LL[g0:, lo:lo + self.n_local].reshape(-1)[first:]
            V = fn(X, ll)
            counts, sums = np.zeros((2, fn.n_out), dtype=np.int64), np.zeros((5, fn.n_out))
            for k in range(fn.n_out):
                cnt, sm = FakeRanks._column(V[:, k])
                counts[:, k], sums[:, k] = cnt[:2], sm
            out.append((counts, sums, len(X), len(X) % self.n_local, V.copy() if values else None))
        return out


def _history(G=11, N=16, d=5, seed=4):
    rs = np.random.RandomState(seed)
    H = rs.normal(size=(G, N, d))
    H[:, :, 2] += 1e8                       # far from the origin, unit spread
    H[3, 5, 1] = 0.0                        # a zero denominator: +-inf
    H[4, 2, 1] = H[4, 2, 2] = 0.0           # 0 / 0: NaN
    LL = -0.5 * (H[:, :, 0] ** 2 + H[:, :, 4] ** 2) - 1e5
    return H, LL


def _py(X, ll, p):
    with np.errstate(all="ignore"):
        return np.stack([X[:, 2] / X[:, 1], X[:, 0] * X[:, 0] + X[:, 4], ll, p[0] + p[1] * X[:, 0], np.zeros(len(X))], axis=1)


FN = HipFunction("""
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[2] / x[1]; out[1] = x[0] * x[0] + x[4]; out[2] = ll; out[3] = p[0] + p[1] * x[0];
}""", n_out=5, params=[0.25, -3.0], python_fn=_py)


def test_check_compiles_without_a_gpu_and_reports_the_compilers_message():
    t = np.linspace(0.0, 1.0, 64)
    good = HipFunction(LINE, n_out=65, params=t)
    assert good.check() and good.check("gfx950") and FN.check()
    with pytest.raises(ValueError, match="does not compile(.|\n)*expected"):
        HipFunction("__device__ void derive(const double* x, int d, double ll, const double* p, double* out) { out[0] = x[0] }", n_out=1).check()
    with pytest.raises(ValueError, match="derive"):                  # the wrapper calls a function the source does not define
        HipFunction("__device__ double other(const double* x) { return x[0]; }", n_out=1).check()
    for bad in (0, 257, -1):
        with pytest.raises(ValueError, match=r"n_out must be 1 \.\.\. 256 \(got %d\)" % bad):
            HipFunction(LINE, n_out=bad)
    with pytest.raises(TypeError, match="n_out must be an integer"):
        HipFunction(LINE, n_out=2.5)
    with pytest.raises(TypeError, match="no python_fn"):
        good(np.zeros((3, 3)), np.zeros(3))
    # the C entry point names its own limit
    import ctypes as C
    from bipymc_amd import _lib as L
    lib = L.load()
    log = C.create_string_buffer(256)
    assert lib.bpm_check_device_function(LINE.encode(), 257, None, log, len(log)) != 0
    assert b"bpm_check_device_function: n_out must be 1 ... 256 (got 257)" in lib.bpm_last_error()


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("n_burn", [0, 3, 16 * 2 + 9, 16 * 11 - 1])
def test_rank_merge_equals_the_pooled_answer_and_values_come_in_super_chain_order(R, n_burn):
    H, LL = _history()
    fr = FakeDeriveRanks(H, LL, R)
    W, wl = H.reshape(-1, fr.d)[n_burn:], LL.reshape(-1)[n_burn:]      # param_est(n_burn)[2] and its log-likelihoods
    V = _py(W, wl, FN.params)
    pd = DV.compute(fr.derive, lambda x: x, FN, n_burn, fr.N, fr.G, values=True)
    assert isinstance(pd, PosteriorDerived)
    assert np.array_equal(pd.values.view(np.uint64), V.view(np.uint64))
    check_summary(pd, V, (R, n_burn))
    assert np.all(pd.mean[4] == 0.0) and np.all(pd.sd[4] == 0.0)        # the output never written
    if n_burn == 0:
        assert pd.n_nan[0] == 1 and np.isnan(pd.mean[0]) and pd.max[0] == np.inf      # 0 / 0 and 1e8 / 0
    no = DV.compute(fr.derive, lambda x: x, FN, n_burn, fr.N, fr.G)
    assert no.values is None
    for f in ("mean", "sd", "min", "max", "n_nan"):
        assert np.array_equal(getattr(no, f), getattr(pd, f), equal_nan=True)
    lo, hi = pd.band(2.0)
    assert np.array_equal(lo, pd.mean - 2.0 * pd.sd, equal_nan=True) and np.array_equal(hi, pd.mean + 2.0 * pd.sd, equal_nan=True)


def test_rank_rows_are_the_super_chain_rows_of_a_ranks_window():
    # 2 ranks of 3 chains, 4 generations, n_burn = 7: generation 1 from chain 1 on -- rank 0 holds chains 1, 2 of it, rank 1 all of its own
    assert DV.rank_rows(0, 2, 6, 4, 2 + 2 * 3, 2).tolist() == [7, 8, 12, 13, 14, 18, 19, 20]
    assert DV.rank_rows(1, 2, 6, 4, 3 * 3, 0).tolist() == [9, 10, 11, 15, 16, 17, 21, 22, 23]
    with pytest.raises(RuntimeError, match="rank 1 reports 7 rows"):
        DV.rank_rows(1, 2, 6, 4, 7, 0)


def test_errors_say_what_is_wrong():
    H, LL = _history()
    fr = FakeDeriveRanks(H, LL, 2)

    def run(fn=FN, n_burn=0, **kw):
        return DV.compute(fr.derive, lambda x: x, fn, n_burn, fr.N, fr.G, **kw)

    with pytest.raises(TypeError, match="param_est_fn: fn must be a HipFunction"):
        run(fn=lambda x: x)
    with pytest.raises(ValueError, match=r"param_est_fn: n_burn must be >= 0 \(got -1\)"):
        run(n_burn=-1)
    with pytest.raises(ValueError, match=r"param_est_fn: the window is empty \(n_burn = 176"):
        run(n_burn=16 * 11)
    with pytest.raises(ValueError, match="window is empty"):
        run(n_burn=10 ** 9)
    assert run(n_burn=16 * 11 - 1).n == 1
    with pytest.raises(ValueError, match="python_fn returned shape"):
        run(fn=HipFunction("", n_out=3, params=[0.0, 1.0], python_fn=_py))
    fr.G = 12                                  # ranks that saw another history than the caller's count of generations
    with pytest.raises(RuntimeError, match="the ranks hold 176 rows of the window"):
        run()
    from bipymc_amd.samplers import DeMc
    with pytest.raises(RuntimeError, match="param_est_fn: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).param_est_fn(FN)
