"""PSIS-LOO with its Pareto-k diagnostic on the GPU (bpm_loo + bipymc_amd/pointwise.py: param_est_loo).

Checks, references and where every bound comes from: tests/_loo_cases.py (the restatements: tests/_psis_restatement.py).  Every call also takes
the matrix L = l_is from param_est_waic(values=True); L is the input of every reference.  Edge sizes come from the layout entry points
(bpm_pointwise_layout, bpm_loo_layout), not from numbers copied here.  Histories are installed (set_history), 16 chains x 130 generations."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _loo_cases as LC  # noqa: E402
import _psis_restatement as PR  # noqa: E402
import _waic_cases as WC  # noqa: E402
from _history_cases import _engine  # noqa: E402

N, G = LC.N, LC.G


def _all(eng, pw, n_burn, r_eff=1.0, what="", fit=True):
    """the device's LOO over the rows >= n_burn against every reference -> (result, L)"""
    w = LC.waic(eng, pw, n_burn)
    L = w.values
    res = LC.loo(eng, pw, n_burn, r_eff)
    LC.check_tails(res, L, r_eff, what)
    LC.check_body(res, L, r_eff, what)
    if fit:
        LC.check_fit(res, L, r_eff, what)
    LC.check_totals(res, w, what)
    return res, L


@pytest.fixture(scope="module")
def narrow():
    e = LC.installed(WC.make_history(G, N, 3))
    yield e
    e.close()


@pytest.fixture(scope="module")
def wide():
    e = LC.installed(WC.make_history(G, N, 640, seed=1))
    yield e
    e.close()


# ---- 1. the tails, exactly (and with them the body and the fit of the same call) ------------------------------------------------------------
@pytest.mark.parametrize("which", ["1", "63", "65", "T", "T+1"])
def test_data_edges(narrow, which):
    T = narrow.pointwise_layout(1, 1)[0]
    n_data = eval(which, {"T": T})
    _all(narrow, WC.pointwise(3, WC.make_data(n_data, 3)), N * G - 226, what="n_data %s" % which, fit=n_data <= 65)


@pytest.mark.parametrize("rows", [1, 5, 21, 224, 226])
def test_window_edges_of_the_tail_length(narrow, rows):
    res, _ = _all(narrow, WC.pointwise(3, WC.make_data(5, 3)), N * G - rows, what="%d rows" % rows)
    assert (res.tail_len == {1: 0, 5: 1, 21: 5, 224: 45, 226: 46}[rows]).all()      # (21: the shortest tail that is fitted)
    if rows <= 5:                                                # a tail of 0 or 1: nothing to fit
        assert (res.tail_len <= 4).all() and (res.pareto_k == np.inf).all() and res.n_bad_k == 5


@pytest.mark.parametrize("past", [0, 1])
def test_the_largest_single_part_window_and_one_row_past_it(narrow, past):
    r_eff = 4.0                                                  # (short kept sets: a part may be as short as four staged tiles)
    full = max(r for r in range(1, N * G + 1) if narrow.loo_layout(r, 5, PR.kept(r, r_eff))[2] == 1)
    assert full < N * G and narrow.loo_layout(full + 1, 5, PR.kept(full + 1, r_eff))[2] == 2
    rows = full + past
    res, _ = _all(narrow, WC.pointwise(3, WC.make_data(5, 3)), N * G - rows, r_eff, what="%d rows, r_eff 4" % rows)
    assert res.stats["tail_parts"] == 1 + past


def test_wide_rows_read_where_they_lie(wide):
    _all(wide, WC.pointwise(3, WC.make_data(5, 3)), N * G - 226, what="d 640")
    rows = N * G
    assert wide.loo_layout(rows, 5, PR.kept(rows, 4.0))[2] == 2
    _all(wide, WC.pointwise(3, WC.make_data(5, 3)), 0, 4.0, what="d 640, two parts")


def test_large_kept_sets_compact_at_least_twice(narrow):
    res, _ = _all(narrow, WC.pointwise(3, WC.make_data(70, 3)), 0, 0.01, what="r_eff 0.01", fit=False)
    assert res.stats["k_max"] == 417 == PR.kept(N * G, 0.01) and res.stats["tail_parts"] == 1
    assert res.stats["compactions"] >= 2, res.stats


def test_r_eff_per_datum_within_one_wavefront(narrow):
    r = np.where(np.arange(65) % 2 == 0, 1.0, 0.25)
    res, _ = _all(narrow, WC.pointwise(3, WC.make_data(65, 3)), N * 3 + 5, r, what="r_eff alternating")
    S = N * G - (N * 3 + 5)
    assert len(res.tails[0]) == PR.kept(S, 1.0) != PR.kept(S, 0.25) == len(res.tails[1])


@pytest.mark.parametrize("order", ["descending", "ascending"])
def test_every_row_appends_or_none_after_the_fill(order):
    e = LC.installed(LC.ordered_history(order))
    pw = WC.pointwise(1, WC.make_data(9, 1), params=LC.ORDER_PARAMS)
    w = LC.waic(e, pw, 0)
    assert (np.diff(w.values, axis=0) < 0).all() if order == "descending" else (np.diff(w.values, axis=0) > 0).all()
    res = LC.loo(e, pw, 0, 0.01)
    LC.check_tails(res, w.values, 0.01, order)
    K = PR.kept(N * G, 0.01)
    # descending: the buffer of 2 K fills every K rows after the first 2 K; ascending: it fills once and nothing is below the threshold again
    assert res.stats["compactions"] == ((N * G - K) // K if order == "descending" else 1), res.stats
    e.close()


def test_duplicated_rows_that_tie_the_cutoff_shorten_the_tail():
    S = N * G
    K = PR.kept(S, 1.0)
    e = LC.installed(LC.ordered_history("shuffled", ties=(K - 3, 6)))      # the values of rank K - 3 ... K + 2 are one value
    pw = WC.pointwise(1, WC.make_data(9, 1), params=LC.ORDER_PARAMS)
    w = LC.waic(e, pw, 0)
    res = LC.loo(e, pw, 0)
    LC.check_tails(res, w.values, 1.0, "ties")
    LC.check_body(res, w.values, 1.0, "ties")
    assert (res.tail_len == K - 3).all() and K - 3 < K - 1                 # M = K - 1
    assert (res.stats["body_n"] == S - (K - 3)).all()
    e.close()


# ---- 3. the fit and the finish; an outlier --------------------------------------------------------------------------------------------------
def test_an_outlier_is_found_by_its_pareto_k():
    n_data, n_burn = 9, 30
    X = WC.make_history(G, N, 3, seed=2)
    Y = WC.make_data(n_data, 4)
    Y[6, 1] += 16.0
    pw = WC.pointwise(4, Y)
    ref = [PR.column(col) for col in pw(X.reshape(-1, 3)[n_burn:]).T]     # the reference alone, on the host
    assert ref[6]["k"] > 0.7 and all(r["k"] < 0.5 for i, r in enumerate(ref) if i != 6)
    e = LC.installed(X)
    res, L = _all(e, pw, n_burn, what="outlier")
    assert res.n_bad_k == 1 and res.pareto_k[6] > 0.7 and (np.delete(res.pareto_k, 6) < 0.5).all()
    text = str(res)
    print(text)
    assert "data with pareto_k > 0.7" in text and "6 (%.3g)" % res.pareto_k[6] in text
    assert [ln for ln in text.splitlines() if ln.startswith("data with pareto_k > 0.7")][0].split()[-1] == "1"
    e.close()


# ---- 4. what is not finite ------------------------------------------------------------------------------------------------------------------
def test_values_that_are_not_finite_stay_in_their_datum():
    n_data, n_burn = 9, 30
    X = WC.make_history(G, N, 3, seed=2)
    flat = X.reshape(-1, 3)
    e = _engine(N, 3)
    rows = N * G - n_burn
    _, _, parts, per_part = e.pointwise_layout(rows, n_data, 4)
    assert parts >= 3
    flat[n_burn:n_burn + per_part, 2] = 7.0
    e.set_history(X, X[-1])
    clean = WC.make_data(n_data, 4)
    Y = clean.copy()
    Y[1, 2], Y[1, 3] = flat[n_burn + per_part, 2], 1.0           # -inf in one row
    Y[2, 2], Y[2, 3] = 7.0, 1.0                                  # -inf in a whole part
    Y[3, 3] = np.inf                                             # -inf in all rows
    Y[4, 2], Y[4, 3] = flat[n_burn + 2 * per_part + 3, 2], -1.0  # one +inf
    Y[5, 2], Y[5, 3] = flat[n_burn + per_part + 100, 2], 0.0     # one NaN
    res, L = _all(e, WC.pointwise(4, Y), n_burn, what="hazards")
    bad = [1, 2, 3, 4, 5]
    assert np.isnan(res.pareto_k[bad]).all() and np.isnan(res.elpd_loo_i[bad]).all() and np.isnan(res.p_loo_i[bad]).all() and (res.tail_len[bad] == 0).all()
    assert res.n_neg_inf.tolist() == [0, 1, per_part, rows, 0, 0, 0, 0, 0] and res.n_pos_inf[4] == 1 and res.n_nan[5] == 1
    assert np.isfinite(res.lppd_i[[1, 2]]).all() and res.lppd_i[3] == -np.inf and res.lppd_i[4] == np.inf and np.isnan(res.lppd_i[5])
    assert np.isnan(res.elpd_loo) and res.n_bad_k == 0
    for i in (1, 2):                                             # the kept set is of the finite values
        fin = L[:, i][np.isfinite(L[:, i])]
        WC.bits_equal(res.tails[i], np.sort(fin)[:PR.kept(rows, 1.0)], ("finite values of datum", i))
    base = LC.loo(e, WC.pointwise(4, clean), n_burn)
    LC.same_loo(res, base, "the data without a planted value", skip=bad)
    e.close()


# ---- 5. stability ---------------------------------------------------------------------------------------------------------------------------
def test_the_same_bits_again_in_small_batches_and_with_new_params(narrow, monkeypatch):
    T = narrow.pointwise_layout(1, 1)[0]
    n_burn = N * (G - 20) + 3
    Y = WC.make_data(2 * T + 17, 3)
    pw = WC.pointwise(3, Y)
    a = LC.loo(narrow, pw, n_burn)
    w = LC.waic(narrow, pw, n_burn)
    LC.check_tails(a, w.values, 1.0, "first")
    LC.check_totals(a, w, "first")
    assert a.stats["batches"] == 1 and a.stats["compiled"] == 1      # (new data: both run-time modules were built)
    again = LC.loo(narrow, pw, n_burn)
    assert again.stats["compiled"] == 0
    LC.same_loo(a, again, "the same call again")
    LC.same_loo(a, LC.loo(narrow, pw, n_burn, tails=False), "without the tails")
    monkeypatch.setenv("BPM_LOO_SCRATCH_MB", "1")
    b = LC.loo(narrow, pw, n_burn)
    assert b.stats["batches"] >= 3 and b.stats["budget_bytes"] == 1 << 20, b.stats
    LC.same_loo(a, b, "three data batches")
    monkeypatch.delenv("BPM_LOO_SCRATCH_MB")
    assert narrow.set_pointwise(pw.source, pw.data, pw.params) is True
    other = WC.pointwise(3, Y, params=[0.25, 1.5, 0.002])
    assert narrow.set_pointwise(other.source, other.data, other.params) is True      # other params: copied, nothing compiled
    c = LC.loo(narrow, other, n_burn)
    assert c.stats["compiled"] == 0                                  # the module of stages A and B was kept too
    LC.check_tails(c, LC.waic(narrow, other, n_burn).values, 1.0, "other params")
    assert not np.array_equal(a.elpd_loo_i, c.elpd_loo_i)
    LC.same_loo(a, LC.loo(narrow, pw, n_burn), "back to the first")


def test_a_closed_sampler_has_given_its_scratch_back(tmp_path):
    """tests/_loo_memory_worker.py in a child process without the runtime's fragment allocator (tests/test_gpu_device_memory.py says why)"""
    out = str(tmp_path / "diff.txt")
    env = dict(os.environ)
    env["HSA_DISABLE_FRAGMENT_ALLOCATOR"] = "1"
    subprocess.check_call(["timeout", "-k", "10", "60", sys.executable, os.path.join(HERE, "_loo_memory_worker.py"), out], env=env, timeout=90)
    diff = int(open(out).read())
    print("free device memory after - before: %d bytes" % diff)
    assert diff == 0


# ---- 6. through the classes; comparison; errors ---------------------------------------------------------------------------------------------
PARABOLA = ("__device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p) {\n"
            "    const double r = y[1] - (x[0] + x[1] * y[0] + x[2] * y[0] * y[0]);\n    return -0.5 * r * r * p[0] - 0.5 * p[1];\n}")


def _parabola(Y):
    from bipymc_amd import HipPointwise

    def fn(X, D, p):
        r = D[None, :, 1] - (X[:, 0:1] + X[:, 1:2] * D[None, :, 0] + X[:, 2:3] * D[None, :, 0] * D[None, :, 0])
        return -0.5 * r * r * p[0] - 0.5 * p[1]
    return HipPointwise(PARABOLA, data=Y, params=[4.0, 0.45], python_fn=fn)


def _check_sampler(s, pw, n_burn):
    w = s.param_est_waic(pw, n_burn, values=True)
    WC.bits_equal(w.values, pw(s.param_est(n_burn)[2]), "values")
    res = s.param_est_loo(pw, n_burn, tails=True)
    LC.check_tails(res, w.values, 1.0, type(s).__name__)
    LC.check_body(res, w.values, 1.0, type(s).__name__)
    LC.check_totals(res, w, type(s).__name__)
    LC.same_loo(res, s.param_est_loo(pw, n_burn, tails=True), "again")
    assert s.param_est_loo(pw, n_burn).tails is None
    return res


@pytest.mark.parametrize("thin", [1, 2])
def test_through_the_sampler_classes(thin):
    from test_gpu_waic import LINE_LIKE, _line_data
    from bipymc_amd import DeMcMpi, DreamMpi, HipFunction, HipLikelihood, compare_loo
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    Y = _line_data()[:40]
    pw = WC.pointwise(3, Y)
    t = d100_gauss.Gauss_100D(rho=0.3, dim=3)
    kw = dict(thin=thin) if thin > 1 else {}
    gens = 20 * thin
    s = DreamMpi(t.ln_like, np.zeros(3), n_chains=N, n_cr_gen=4, burnin_gen=8, seed=21, **kw)
    s.run_mcmc(N * (gens + 1))
    a = _check_sampler(s, pw, N * 3 + 5)
    if thin > 1:
        return
    b = _check_sampler(s, _parabola(Y), N * 3 + 5)
    diff, se = compare_loo(a, b)
    with np.errstate(invalid="ignore"):
        d = a.elpd_loo_i - b.elpd_loo_i
        WC.bits_equal([diff, se], [a.elpd_loo - b.elpd_loo, np.sqrt(len(d) * np.var(d))], "compare_loo")
    twice = HipFunction("__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {\n"
                        "    for (int k = 0; k < 3; ++k) out[k] = 2.0 * x[k];\n}", n_out=3)
    with s.derived_history(twice) as dh:
        _check_sampler(dh, pw, N * 3 + 5)
    s = DeMcMpi(t.ln_like, np.zeros(3), n_chains=N, seed=5)
    s.run_mcmc(N * (gens + 1))
    _check_sampler(s, pw, N * 2 + 1)
    like = HipLikelihood(LINE_LIKE, params=[4.0], terms=1, data=_line_data())
    s = DeMc(like, n_chains=N, seed=8)
    s.run_mcmc(N * gens, np.array([1.0, 2.0, 0.0]))
    _check_sampler(s, pw, N * 4 + 7)


def test_errors_say_what_is_wrong(narrow, monkeypatch):
    from bipymc_amd import _lib as L
    from bipymc_amd import PosteriorLoo, compare_loo
    from bipymc_amd import pointwise as PW
    pw = WC.pointwise(1, WC.make_data(4, 1))
    with pytest.raises(NotImplementedError, match=r"param_est_loo: .* single rank only \(this communicator has 2 ranks\)"):
        PW.compute_loo(narrow, lambda obj: [obj, obj], pw, 0, narrow.n_chains)
    with pytest.raises(ValueError, match="param_est_loo: the window is empty"):
        LC.loo(narrow, pw, N * G)
    assert LC.loo(narrow, pw, N * G - 1).n == 1
    for bad in ([1.0, 1.0], 0.0, -1.0, np.nan, [1.0, 1.0, np.inf, 1.0]):
        with pytest.raises(ValueError, match="param_est_loo: r_eff must be"):
            LC.loo(narrow, pw, 0, bad)
    assert LC.loo(narrow, pw, 0, 2.5).n == N * G                 # above 1 is legal
    with pytest.raises(TypeError, match="param_est_loo: pw must be a HipPointwise"):
        LC.loo(narrow, "pw", 0)
    # a kept set that does not fit the budget is refused with advice before bpm_loo compiles its module or allocates any scratch
    fresh = _engine(N, 3)
    X = WC.make_history(G, N, 3)
    fresh.set_history(X, X[-1])
    monkeypatch.setenv("BPM_LOO_SCRATCH_MB", "0")
    with pytest.raises(L.BpmError, match=r"bpm_loo: the kept sets of one tile of 256 data \(138 of 2080 draws each\) need \d+ bytes of scratch; the budget is 0 bytes "
                                         r"\(BPM_LOO_SCRATCH_MB(.|\n)*raise r_eff towards 1, shorten the window with n_burn, or thin the history"):
        LC.loo(fresh, pw, 0)
    monkeypatch.delenv("BPM_LOO_SCRATCH_MB")
    assert LC.loo(fresh, pw, 0).n == N * G
    fresh.close()
    a = LC.loo(narrow, pw, 0)
    assert isinstance(a, PosteriorLoo)
    with pytest.raises(TypeError, match="compare_loo: both arguments must be PosteriorLoo"):
        compare_loo(a, LC.waic(narrow, pw, 0))
    with pytest.raises(ValueError, match="compare_loo: the results are over 2080 and 2079 draws"):
        compare_loo(a, LC.loo(narrow, pw, 1))
    with pytest.raises(ValueError, match="compare_loo: the results are over 4 and 5 data points"):
        compare_loo(a, LC.loo(narrow, WC.pointwise(1, WC.make_data(5, 1)), 0))
