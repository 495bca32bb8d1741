"""Posterior summaries of user-written derived quantities on the GPU (bpm_set_device_function / bpm_derive + bipymc_amd/derived.py).

Reference: NumPy on what get_history / get_loglike_history return, restricted to param_est's rows (the super-chain rows >= n_burn).  With a
derive built from + - * / only (IEEE-exact under -ffp-contract=off) the values equal the NumPy statement bit for bit -- except that where
both are NaN only that is compared: IEEE 754 leaves sign and payload of a NaN an operation creates (0 / 0, inf - inf) to the implementation,
and x86 and the GPU choose differently.  min, max, n_nan and n are exact; mean and sd lie within trace_bound(n, max |v|, max |v - m|)
(tests/test_traces_host.py: derived for any summation order) of a np.longdouble evaluation of those values; a function with exp is compared
at the project's float tolerance of 1e-12 relative."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from _history_cases import _dream_class, _engine, group_single_rank, local_group, per_rank  # noqa: E402
from test_derived_host import check_summary  # noqa: E402
from test_gpu_traces import _installed  # noqa: E402

FIVE_SRC = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[2] / x[1];
    out[1] = x[0] * x[0] + x[4];
    out[2] = ll;
    out[3] = p[0] + p[1] * x[0];      // out[4] is never written
}"""
EXP_SRC = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = exp(-0.5 * x[0] * x[0]);
    out[1] = x[2] / x[1];
}"""
WIDE_SRC = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = x[d - 1] - x[0];
    out[1] = x[1] * x[d - 2];
    out[2] = ll * p[0];
}"""


def _five_py(X, ll, p):
    with np.errstate(all="ignore"):
        return np.stack([X[:, 2] / X[:, 1], X[:, 0] * X[:, 0] + X[:, 4], ll, p[0] + p[1] * X[:, 0], np.zeros(len(X))], axis=1)


def _five():
    from bipymc_amd import HipFunction
    return HipFunction(FIVE_SRC, n_out=5, params=[0.25, -3.0], python_fn=_five_py)


def _layout(M, params=()):
    """out[m] = x[m % d] * (m + 1), m < M"""
    from bipymc_amd import HipFunction

    def py(X, ll, p):
        with np.errstate(all="ignore"):
            return np.stack([X[:, m % X.shape[1]] * (m + 1) for m in range(M)], axis=1)

    return HipFunction("__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {\n"
                       "    for (int m = 0; m < %d; ++m) out[m] = x[m %% d] * (m + 1);\n}" % M, n_out=M, params=params, python_fn=py)


def _device(eng, fn, n_burn=0, values=True):
    from bipymc_amd import derived as DV
    return DV.compute(eng.derive, DV.single_process_allgather, fn, n_burn, eng.n_chains, eng.history_rows(), values=values)


def _bits_equal(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    both_nan = np.isnan(a) & np.isnan(b)
    bad = (a.view(np.uint64) != b.view(np.uint64)) & ~both_nan
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), a[bad][:4], b[bad][:4])


def _same_bits(a, b):
    assert a._fields == b._fields
    for f, x, y in zip(a._fields, a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, f
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y), f


def _check(pd, fn, H, LL, n_burn, exact=None, what=""):
    """pd against fn's NumPy statement on the rows >= n_burn of the history H (G, N, d) with log-likelihoods LL (G, N); exact: the outputs
    compared bit for bit (default all), the others at 1e-12 relative"""
    d = H.shape[-1]
    X, ll = H.reshape(-1, d)[n_burn:], LL.reshape(-1)[n_burn:]
    V = fn(X, ll)
    cols = list(range(fn.n_out)) if exact is None else list(exact)
    assert pd.n == len(X) and pd.values.shape == V.shape, (what, pd.n, len(X))
    _bits_equal(pd.values[:, cols], V[:, cols], what)
    for k in set(range(fn.n_out)) - set(cols):
        assert np.allclose(pd.values[:, k], V[:, k], rtol=1e-12, atol=0.0, equal_nan=True), (what, k)
    check_summary(pd, pd.values, what)          # min, max, n_nan, n exactly; mean and sd within the bound of those values
    return V


def _history_with_zero_denominators():
    X = _installed()                            # a constant column, a 1e8 offset, denormals, NaN, +-inf
    X[20, 5, 1] = 0.0                           # x2 / 0: +inf
    X[21, 7, 1] = -0.0                          # x2 / -0: -inf
    X[22, 9, 1] = X[22, 9, 2] = 0.0             # 0 / 0: NaN
    return X


@pytest.fixture(scope="module")
def installed():
    X = _history_with_zero_denominators()
    G, N, d = X.shape
    e = _engine(N, d)
    e.set_history(X, X[-1])
    H, LL = e.get_history(), e.get_loglike_history()
    assert np.array_equal(H, X, equal_nan=True)
    yield e, H, LL
    e.close()


@pytest.mark.parametrize("n_burn", [0, 3, 256 * 5 + 1, 256 * 40 - 1])
def test_installed_history_against_numpy(installed, n_burn):
    e, H, LL = installed
    fn = _five()
    pd = _device(e, fn, n_burn)
    V = _check(pd, fn, H, LL, n_burn, what=n_burn)
    assert pd.n == 256 * 40 - n_burn
    assert np.all(pd.values[:, 4] == 0.0) and pd.mean[4] == 0.0 and pd.sd[4] == 0.0 and pd.min[4] == 0.0 and pd.max[4] == 0.0
    if n_burn <= 256 * 5 + 1:
        assert pd.max[0] == np.inf and pd.min[0] == -np.inf and pd.n_nan[0] == 1 and np.isnan(pd.mean[0]) and np.isnan(pd.sd[0])
        assert pd.n_nan[1] == int(np.isnan(V[:, 1]).sum()) > 256
    no = _device(e, fn, n_burn, values=False)
    assert no.values is None
    _same_bits(no._replace(values=0.0), pd._replace(values=0.0))


@pytest.mark.parametrize("M,params", [(1, [2.0]), (3, []), (256, [1.0, 2.0, 3.0])])
def test_lane_layouts_and_replacing_the_function_on_one_handle(installed, M, params):
    """n_out = 1: 256 lanes merge into one output; 3: cpw = 85, no power of two; 256: one lane per output, the largest output tile.  Each is
    another source and another n_out on the handle that held the previous one."""
    e, H, LL = installed
    fn = _layout(M, params)
    for n_burn in (3, 256 * 40 - 1):
        _check(_device(e, fn, n_burn), fn, H, LL, n_burn, what=(M, n_burn))
    five = _five()                               # ... and back to another source with another n_out
    _check(_device(e, five, 256 * 38 + 5), five, H, LL, 256 * 38 + 5, what="five again")


def test_several_workgroups_ragged_last_part_and_two_libraries_in_one_process(installed):
    """N = 4096, G = 64, n_burn = 4096 * 3 + 1: 244 workgroups of 1024 rows, the last one 1023.  That engine runs on the test variant of the
    library while the module's installed engine (the product library) holds another function: each launches its own module's kernel."""
    from bipymc_amd import _lib as L
    e0, H0, LL0 = installed
    lay = _layout(3)
    _check(_device(e0, lay, 5), lay, H0, LL0, 5, what="product, before")
    N, d, G = 4096, 7, 64
    rs = np.random.RandomState(3)
    X = rs.normal(size=(G, N, d)) * np.arange(1, d + 1)
    X[:, :, 2] += 1e8
    X[10:12, 1000:3000, 4] = np.nan
    X[50, 4000, 0] = -np.inf
    e = _engine(N, d, lib=L.load_test())
    e.set_history(X, X[-1])
    H, LL = e.get_history(), e.get_loglike_history()
    fn = _five()
    n_burn = N * 3 + 1
    pd = _device(e, fn, n_burn)
    _check(pd, fn, H, LL, n_burn, what="test variant")
    _same_bits(pd, _device(e, fn, n_burn))
    _check(_device(e0, lay, 5), lay, H0, LL0, 5, what="product, after")       # (reuses its loaded module)
    _check(_device(e, fn, N * 63 + 7), fn, H, LL, N * 63 + 7, what="test variant, again")
    e.close()


def _check_sampler(s, fn, n_burn, exact=None):
    pd = s.param_est_fn(fn, n_burn, values=True)            # (first: a history in position order is put into chain order here)
    W = s.param_est(0)[2]
    N = s.n_chains
    H = W.reshape(W.shape[0] // N, N, -1)
    LL = s._engine.get_loglike_history()
    assert np.array_equal(H, s._engine.get_history())
    _check(pd, fn, H, LL, n_burn, exact=exact)
    _same_bits(pd, s.param_est_fn(fn, n_burn, values=True))
    assert np.array_equal(s.param_est(0)[2], W)
    return pd


def test_wide_rows_are_read_where_they_lie():
    from bipymc_amd import HipFunction
    s = _dream_class(64, 640, 30)

    def py(X, ll, p):
        return np.stack([X[:, -1] - X[:, 0], X[:, 1] * X[:, -2], ll * p[0]], axis=1)

    _check_sampler(s, HipFunction(WIDE_SRC, n_out=3, params=[-2.0], python_fn=py), 64 * 2 + 1)


def test_dream_shuffled_history_in_position_order():
    s = _dream_class(256, 10, 60)
    _check_sampler(s, _five(), 256 * 4 + 9)


def test_serial_demc_and_a_function_with_exp():
    from bipymc_amd import HipFunction
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.3, dim=6)
    s = DeMc(t.ln_like, n_chains=64, seed=8)
    s.run_mcmc(64 * 100, np.zeros(6))

    def py(X, ll, p):
        return np.stack([np.exp(-0.5 * X[:, 0] * X[:, 0]), X[:, 2] / X[:, 1]], axis=1)

    pd = _check_sampler(s, HipFunction(EXP_SRC, n_out=2, python_fn=py), 64 * 5 + 1, exact=[1])
    assert 0.0 < pd.min[0] <= pd.mean[0] <= pd.max[0] <= 1.0


def test_local_group_equals_single_rank():
    from bipymc_amd import derived as DV
    fn = _five()
    ranks, N, d = local_group(2)
    n_burn = N * 7 + N // 2 + 1                                   # the partial generation starts inside the second rank's chains
    G = ranks[0].history_rows()
    res = DV.compute(per_rank(ranks, "derive"), lambda x: x, fn, n_burn, N, G, values=True)
    res3 = DV.compute(per_rank(ranks, "derive"), lambda x: x, fn, 3, N, G, values=True)       # ... and inside the first rank's
    for e in ranks:
        e.close()
    one = group_single_rank()
    ref, ref3 = _device(one, fn, n_burn), _device(one, fn, 3)
    H, LL = one.get_history(), one.get_loglike_history()
    one.close()
    for a, b, nb in ((res, ref, n_burn), (res3, ref3, 3)):
        _check(b, fn, H, LL, nb, what="one rank")
        _check(a, fn, H, LL, nb, what="two ranks")              # (mean and sd each within the bound of the exact value)
        _same_bits(a._replace(mean=0.0, sd=0.0), b._replace(mean=0.0, sd=0.0))


def test_no_side_effects():
    fn, lay = _five(), _layout(3)
    a = _engine(256, 12)
    a.set_state(np.random.RandomState(1).normal(size=(256, 12)))
    a.begin_run()
    a.step(100)
    r1 = _device(a, fn, 256 * 3 + 9)
    _same_bits(r1, _device(a, fn, 256 * 3 + 9))
    a.step(50)
    _device(a, lay, 7, values=False)
    a.step(50)
    _device(a, fn, 0)
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
    import ctypes as C
    from bipymc_amd import HipFunction
    from bipymc_amd import _lib as L
    fn = _five()
    e = _engine(64, 5, burnin_gen=0, keep_history=False)
    e.set_state(np.zeros((64, 5)) + np.arange(5))
    e.begin_run()
    e.step(10)
    with pytest.raises(L.BpmError, match="bpm_derive: needs keep_history=True"):
        _device(e, fn, 0)
    e.close()
    e = _engine(64, 5)
    e.set_state(np.random.RandomState(2).normal(size=(64, 5)))
    e.begin_run()
    e.step(20)
    with pytest.raises(L.BpmError, match=r"bpm_derive: no device function installed \(bpm_set_device_function\)"):
        e.derive_rows(0)
    with pytest.raises(L.BpmError, match="bpm_set_device_function: the function source does not compile(.|\n)*expected"):
        _device(e, HipFunction("__device__ void derive(const double* x, int d, double ll, const double* p, double* out) { out[0] = x[0] }", n_out=1), 0)
    with pytest.raises(L.BpmError, match=r"bpm_set_device_function: n_out must be 1 \.\.\. 256 \(got 0\)"):
        e.set_device_function(FIVE_SRC, 0)
    with pytest.raises(TypeError, match="param_est_fn: fn must be a HipFunction"):
        _device(e, FIVE_SRC, 0)
    with pytest.raises(ValueError, match="param_est_fn: n_burn must be >= 0"):
        _device(e, fn, -1)
    with pytest.raises(ValueError, match="param_est_fn: the window is empty"):
        _device(e, fn, 21 * 64)
    assert _device(e, fn, 21 * 64 - 1).n == 1
    # the C entry point names its own limits
    counts = np.zeros((2, 5), dtype=np.int64); sums = np.zeros((5, 5)); buf = np.empty(64 * 5)
    n_rows, n_first = C.c_int64(0), C.c_int64(0)
    i64, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)

    def derive(n_burn, cap):
        e._ck(e.lib.bpm_derive(e._h, n_burn, counts.ctypes.data_as(i64), sums.ctypes.data_as(dp), C.byref(n_rows), C.byref(n_first),
                               buf.ctypes.data_as(dp), cap))

    with pytest.raises(L.BpmError, match=r"bpm_derive: values holds 319 doubles; the window needs 320"):
        derive(20 * 64, 319)
    derive(20 * 64, 320)
    assert n_rows.value == 64 and n_first.value == 0
    derive(20 * 64 + 60, 320)
    assert n_rows.value == 4 and n_first.value == 4
    with pytest.raises(L.BpmError, match=r"bpm_derive: n_burn must be >= 0 \(got -1\)"):
        derive(-1, 320)
    e.close()
    from bipymc_amd.samplers import DeMc
    with pytest.raises(RuntimeError, match="param_est_fn: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).param_est_fn(fn)
