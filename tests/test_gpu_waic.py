"""WAIC and the pointwise log predictive density on the GPU (bpm_set_pointwise / bpm_pointwise + bipymc_amd/pointwise.py).

Functions, exact reference, bounds (derived, with the one measured constant E) and the checker: tests/_waic_cases.py.  Every call asks for
the values too: they must equal python_fn's matrix bit for bit, and the reductions are compared with the exact reduction of that matrix.
Edge sizes come from bpm_pointwise_layout (T, rows per tile R, parts, rows per part), not from numbers copied here.  Histories are installed
(set_history), 16 chains, so that a window of any number of rows is an n_burn away."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _waic_cases as WC  # noqa: E402
from _history_cases import _engine  # noqa: E402

N, G = 16, 130            # 2080 rows


def _device(eng, pw, n_burn=0, values=True):
    from bipymc_amd import pointwise as PW
    return PW.compute(eng.pointwise, PW.single_process_allgather, pw, n_burn, eng.n_chains, eng.history_rows(), values=values)


def _check(eng, pw, H, n_burn, what, ref=None):
    """the device's result over the rows >= n_burn of the history H (G, N, d) against the exact reduction of python_fn's matrix
    -> (result, matrix, reference)"""
    L = pw(H.reshape(-1, H.shape[2])[n_burn:])
    T, R, parts, per_part = eng.pointwise_layout(len(L), pw.n_data, pw.w)
    res = _device(eng, pw, n_burn)
    WC.bits_equal(res.values, L, (what, "values"))
    ref = WC.check_result(res, L, per_part, parts, ref=ref, what=what)
    return res, L, ref


def _installed(d, seed=0):
    X = WC.make_history(G, N, d, seed=seed)
    e = _engine(N, d)
    e.set_history(X, X[-1])
    H = e.get_history()
    assert np.array_equal(H, X)
    return e, H


@pytest.fixture(scope="module")
def narrow():
    e, H = _installed(3)
    yield e, H
    e.close()


@pytest.fixture(scope="module")
def wide():
    e, H = _installed(640, seed=1)
    yield e, H
    e.close()


def _tile(eng):
    return eng.pointwise_layout(1, 1)[0]


@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("which", ["1", "63", "64", "65", "T-1", "T", "T+1", "2*T+17"])
def test_data_edges_every_datum_gets_its_own_values(narrow, which, w):
    e, H = narrow
    T = _tile(e)
    n_data = eval(which, {"T": T})
    n_burn = N * (G - 4) + 5                                     # 59 rows, a partial first generation
    _check(e, WC.pointwise(w, WC.make_data(n_data, w)), H, n_burn, "n_data %s = %d, w %d" % (which, n_data, w))


def test_data_read_where_they_lie_above_the_register_cut_off(narrow):
    e, H = narrow
    T = _tile(e)
    _check(e, WC.pointwise(9, WC.make_data(T + 1, 9)), H, N * (G - 3) + 1, "w 9, n_data T + 1")


def _row_edges(eng, n_data):
    """window sizes: 1, R - 1, R, R + 1, the largest single part, one row past it, the smallest giving >= 3 parts with a shorter last one"""
    T, R, _, _ = eng.pointwise_layout(1, n_data)
    full = max(r for r in range(1, N * G + 1) if eng.pointwise_layout(r, n_data)[2] == 1)
    three = min(r for r in range(full + 1, N * G + 1) if eng.pointwise_layout(r, n_data)[2] >= 3 and eng.pointwise_layout(r, n_data)[2] * eng.pointwise_layout(r, n_data)[3] != r)
    assert full < three <= N * G and eng.pointwise_layout(full + 1, n_data)[2] == 2
    return R, [1, R - 1, R, R + 1, full, full + 1, three]


@pytest.mark.parametrize("k", range(7))
def test_row_edges_staged_rows(narrow, k):
    e, H = narrow
    pw = WC.pointwise(3, WC.make_data(5, 3))
    R, rows = _row_edges(e, 5)
    n_burn = N * G - rows[k]                                     # (1 leaves one row; R - 1, R + 1, ... are no multiples of 16: a partial first generation)
    _, _, parts, per_part = e.pointwise_layout(rows[k], 5)
    _check(e, pw, H, n_burn, "d 3: %d rows (R %d, %d parts of %d)" % (rows[k], R, parts, per_part))


@pytest.mark.parametrize("k", [0, 1, 3, 5, 6])
def test_row_edges_wide_rows_read_where_they_lie(wide, k):
    e, H = wide
    pw = WC.pointwise(3, WC.make_data(5, 3))                     # (reads x[d - 1] = x[639])
    R, rows = _row_edges(e, 5)
    _, _, parts, per_part = e.pointwise_layout(rows[k], 5)
    _check(e, pw, H, N * G - rows[k], "d 640: %d rows (%d parts of %d)" % (rows[k], parts, per_part))


def test_log_sum_exp_hazards_follow_the_rules_and_stay_in_their_datum():
    n_data = 9
    X = WC.make_history(G, N, 3, seed=2)
    flat = X.reshape(-1, 3)
    e = _engine(N, 3)
    rows = N * G - 30
    T, R, parts, per_part = e.pointwise_layout(rows, n_data, 4)
    assert parts >= 3
    n_burn = 30
    flat[n_burn:n_burn + per_part, 2] = 7.0                      # every row of part 0 holds the same x[2]
    e.set_history(X, X[-1])
    H = e.get_history()
    clean = WC.make_data(n_data, 4)
    Y = clean.copy()
    Y[1, 2], Y[1, 3] = flat[n_burn + per_part, 2], 1.0           # -inf at the first row of part 1
    Y[2, 2], Y[2, 3] = 7.0, 1.0                                  # -inf at every row of part 0 (its first row included), finite elsewhere
    Y[3, 3] = np.inf                                             # -inf at every row
    Y[4, 2], Y[4, 3] = flat[n_burn + 2 * per_part + 3, 2], -1.0  # one +inf
    Y[5, 2], Y[5, 3] = flat[n_burn + per_part + 100, 2], 0.0     # one NaN (0 / 0), in part 1
    Y[6, 1] = 3000.0                                             # log densities spread over more than 1500
    res, L, _ = _check(e, WC.pointwise(4, Y), H, n_burn, "hazards")
    assert L[per_part, 1] == -np.inf and (L[:, 1] == -np.inf).sum() == 1
    assert (L[:per_part, 2] == -np.inf).all() and np.isfinite(L[per_part:, 2]).all()
    assert (L[:, 3] == -np.inf).all() and (L[:, 4] == np.inf).sum() == 1 and np.isnan(L[:, 5]).sum() == 1
    assert np.isfinite(L[:, 6]).all() and L[:, 6].max() - L[:, 6].min() > 1500.0
    assert np.isfinite(res.lppd_i[[1, 2, 6]]).all() and np.isnan(res.p_waic_i[[1, 2]]).all() and (res.mean_i[[1, 2, 3]] == -np.inf).all()
    assert res.lppd_i[3] == -np.inf and res.lppd_i[4] == np.inf and np.isnan([res.lppd_i[5], res.p_waic_i[5], res.mean_i[5]]).all()
    assert res.n_neg_inf.tolist() == [0, 1, per_part, rows, 0, 0, 0, 0, 0] and res.n_pos_inf[4] == 1 and res.n_nan[5] == 1
    base = _device(e, WC.pointwise(4, clean), n_burn)
    WC.same_result(res, base, "the data without a planted value", skip=[1, 2, 3, 4, 5, 6])
    e.close()


def test_stability_params_without_recompile_and_another_w_on_the_same_handle(narrow):
    e, H = narrow
    n_burn = N * (G - 20) + 3
    Y = WC.make_data(70, 3)
    pw = WC.pointwise(3, Y)
    a, _, ref = _check(e, pw, H, n_burn, "first")
    WC.same_result(a, _device(e, pw, n_burn), "the same call again")
    WC.same_result(a, _device(e, pw, n_burn, values=False), "without the values")
    assert e.set_pointwise(pw.source, pw.data, pw.params) is True             # the same source, w and data: kept
    other = WC.pointwise(3, Y, params=[0.25, 1.5, 0.002])
    assert e.set_pointwise(other.source, other.data, other.params) is True    # other params: copied, nothing compiled
    b, _, _ = _check(e, other, H, n_burn, "other params")
    assert not np.array_equal(a.lppd_i, b.lppd_i)
    Y2 = Y.copy()
    Y2[69, 1] += 1.0
    assert e.set_pointwise(pw.source, Y2, pw.params) is False                 # other data: installed anew
    _check(e, WC.pointwise(1, WC.make_data(70, 1)), H, n_burn, "w 1 replaces w 3")
    _check(e, WC.pointwise(9, WC.make_data(33, 9)), H, n_burn, "w 9 replaces w 1")
    c, _, _ = _check(e, pw, H, n_burn, "back to the first", ref=ref)
    WC.same_result(a, c, "back to the first")


def test_values_of_two_to_the_31_elements_are_refused_before_anything_is_allocated(narrow):
    e, H = narrow
    n_data = (1 << 31) // (N * G) + 1
    from bipymc_amd import HipPointwise
    big = HipPointwise(WC.SOURCES[1], data=np.zeros(n_data), params=WC.PARAMS)
    was = getattr(e, "_pointwise_n_data", None)
    with pytest.raises(ValueError, match=r"param_est_waic: the values of 2080 rows x %d data points are %d elements; fewer than 2\^31 per rank can be returned"
                       % (n_data, 2080 * n_data)):
        _device(e, big, 0)
    assert getattr(e, "_pointwise_n_data", None) == was                      # nothing was installed


def test_errors_say_what_is_wrong(narrow):
    from bipymc_amd import HipPointwise
    from bipymc_amd import _lib as L
    e, H = narrow
    with pytest.raises(L.BpmError, match="bpm_set_pointwise: the pointwise source does not compile(.|\n)*ln_like_point"):
        _device(e, HipPointwise("__device__ double f(double a) { return a; }", data=np.zeros(4)), 0)
    f = _engine(N, 3)
    with pytest.raises(L.BpmError, match=r"bpm_pointwise: no pointwise function installed \(bpm_set_pointwise\)"):
        f.pointwise_rows(0)
    f.close()
    pw = WC.pointwise(1, WC.make_data(4, 1))
    with pytest.raises(ValueError, match="param_est_waic: the window is empty"):
        _device(e, pw, N * G)
    assert _device(e, pw, N * G - 1).n == 1


def test_a_closed_sampler_has_given_its_data_back(tmp_path):
    """tests/_waic_memory_worker.py in a child process without the runtime's fragment allocator (tests/test_gpu_device_memory.py says why):
    the free device memory after a sampler with a pointwise function and 4 MiB of data was closed equals the free memory before"""
    out = str(tmp_path / "diff.txt")
    env = dict(os.environ)
    env["HSA_DISABLE_FRAGMENT_ALLOCATOR"] = "1"
    subprocess.check_call(["timeout", "-k", "10", "60", sys.executable, os.path.join(HERE, "_waic_memory_worker.py"), out], env=env, timeout=90)
    diff = int(open(out).read())
    print("free device memory after - before: %d bytes" % diff)
    assert diff == 0


LINE_LIKE = """
__device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc) {
    const double r = y[1] - (x[0] + x[1] * y[0]);
    acc[0] += r * r;
}
__device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p) {
    return -0.5 * acc[0] * p[0] - 0.5 * x[2] * x[2];
}"""


def _line_data():
    rs = np.random.RandomState(77)
    t = rs.uniform(0.0, 1.0, size=200)
    return np.column_stack([t, 1.0 + 2.0 * t + 0.5 * rs.normal(size=200), rs.normal(size=200)])


def _check_sampler(s, pw, n_burn):
    res = s.param_est_waic(pw, n_burn, values=True)
    W = s.param_est(n_burn)[2]                                   # the window: stored rows of a thinned history
    L = pw(W)
    T, R, parts, per_part = s._engine.pointwise_layout(len(W), pw.n_data, pw.w)
    WC.bits_equal(res.values, L, "values")
    WC.check_result(res, L, per_part, parts, what=type(s).__name__)
    WC.same_result(res, s.param_est_waic(pw, n_burn, values=True))
    return res


@pytest.mark.parametrize("thin", [1, 2])
def test_through_the_sampler_classes(thin):
    from bipymc_amd import DeMcMpi, DreamMpi, HipLikelihood
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    Y = _line_data()
    pw = WC.pointwise(3, Y)
    t = d100_gauss.Gauss_100D(rho=0.3, dim=3)
    kw = dict(thin=thin) if thin > 1 else {}
    gens = 20 * thin
    s = DreamMpi(t.ln_like, np.zeros(3), n_chains=N, n_cr_gen=4, burnin_gen=8, seed=21, **kw)
    s.run_mcmc(N * (gens + 1))
    _check_sampler(s, pw, N * 3 + 5)
    if thin > 1:
        return
    # a DerivedHistory inherits the method: the pointwise density of the derived quantities (here twice the parameters) as rows
    from bipymc_amd import HipFunction
    twice = HipFunction("__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {\n"
                        "    for (int k = 0; k < 3; ++k) out[k] = 2.0 * x[k];\n}", n_out=3)
    with s.derived_history(twice) as dh:
        assert np.array_equal(dh.param_est(0)[2], 2.0 * s.param_est(0)[2])
        _check_sampler(dh, pw, N * 3 + 5)
    s = DeMcMpi(t.ln_like, np.zeros(3), n_chains=N, seed=5)
    s.run_mcmc(N * (gens + 1))
    _check_sampler(s, pw, N * 2 + 1)
    like = HipLikelihood(LINE_LIKE, params=[4.0], terms=1, data=Y)
    s = DeMc(like, n_chains=N, seed=8)
    s.run_mcmc(N * gens, np.array([1.0, 2.0, 0.0]))
    _check_sampler(s, pw, N * 4 + 7)
