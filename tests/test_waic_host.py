"""bipymc_amd/pointwise.py without a GPU: HipPointwise's validation and compile-only check (hiprtc builds bpm_pointwise_rows of
bipymc_amd/csrc/pointwise_rows.h around the caller's function for gfx950), pointwise.compute driven by a NumPy stand-in for the device call
on 1 and 3 emulated ranks of unequal share, the merge formulas on records with empty parts and values that are not finite, the rules for
those values against SciPy / NumPy, compare_waic, and the stand-alone sanitizer program of the host-side arithmetic.

Reference and bounds: tests/_waic_cases.py."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _waic_cases as WC  # noqa: E402
from bipymc_amd import HipPointwise, PosteriorWaic, compare_waic  # noqa: E402
from bipymc_amd import pointwise as PW  # noqa: E402


def _reduce(L):
    """what a rank hands over for its matrix L (rows, n_data): counts (4, n_data), sums (5, n_data) -- the device's record, by NumPy"""
    nd = L.shape[1]
    counts, sums = np.zeros((4, nd), dtype=np.int64), np.zeros((5, nd))
    sums[3] = -np.inf
    for k in range(nd):
        col = L[:, k]
        fin = col[np.isfinite(col)]
        counts[:, k] = len(fin), np.isnan(col).sum(), (col == np.inf).sum(), (col == -np.inf).sum()
        if len(fin):
            c, m = fin[0], fin.max()
            sums[:, k] = c, np.sum(fin - c), np.sum((fin - c) ** 2), m, np.sum(np.exp(fin - m))
    return counts, sums


class FakePointwiseRanks(object):
    """bpm_pointwise of ranks that hold shares[r] consecutive chains each of the history H (G, N, d): pw's python_fn over the rank's rows of
    param_est's window, reduced by NumPy.  (derived.rank_rows wants equal shares: unequal ones go without values.)"""

    def __init__(self, H, shares):
        self.H = np.asarray(H, dtype=np.float64)
        self.G, self.N, self.d = self.H.shape
        self.shares = list(shares)
        assert sum(self.shares) == self.N

    def pointwise(self, pw, n_burn, values):
        out, lo = [], 0
        for n_local in self.shares:
            g0 = n_burn // self.N
            first = min(max(n_burn % self.N - lo, 0), n_local)
            X = self.H[g0:, lo:lo + n_local].reshape(-1, self.d)[first:]
            L = pw(X) if len(X) else np.zeros((0, pw.n_data))
            counts, sums = _reduce(L)
            out.append((counts, sums, len(X), len(X) % n_local, L.copy() if values else None))
            lo += n_local
        return out


def test_validation_errors_are_hiplikelihoods():
    src = WC.SOURCES[1]
    for bad, msg in ((np.zeros((3, 2), dtype=np.float32), r"data must be float64 \(got float32\)"),
                     (np.zeros((2, 2, 2)), r"data must have shape \(n_data, w\) or \(n_data,\)"),
                     (np.zeros((0, 2)), r"data must have 1 <= n_data < 2\^31 rows \(got 0\)"),
                     (np.zeros((3, 65)), r"data must have 1 <= w <= 64 values per datum \(got 65\)"),
                     (np.zeros((3, 0)), r"data must have 1 <= w <= 64 values per datum \(got 0\)")):
        with pytest.raises(ValueError, match=msg):
            HipPointwise(src, data=bad)
    pw = HipPointwise(src, data=np.arange(5.0), params=[1.0, 2.0, 3.0])
    assert pw.data.shape == (5, 1) and pw.n_data == 5 and pw.w == 1 and pw.params.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(TypeError, match="no python_fn"):
        pw(np.zeros((2, 3)))
    with pytest.raises(ValueError, match="python_fn returned shape"):
        HipPointwise(src, data=np.arange(5.0), python_fn=lambda X, Y, p: np.zeros((len(X), 4)))(np.zeros((2, 3)))


def test_check_compiles_without_a_gpu_and_reports_the_compilers_message():
    for w in sorted(WC.SOURCES):
        assert WC.pointwise(w, WC.make_data(7, w)).check()
    assert WC.pointwise(3, WC.make_data(7, 3)).check("gfx950")
    with pytest.raises(ValueError, match=r"it must define `__device__ double ln_like_point\(const double\* x, int d, const double\* y, int i, const double\* p\)`(.|\n)*ln_like_point"):
        HipPointwise("__device__ double other(const double* x) { return x[0]; }", data=np.zeros(3)).check()
    with pytest.raises(ValueError, match="does not compile(.|\n)*expected"):
        HipPointwise(WC.SOURCES[1].replace("p[2];", "p[2]"), data=np.zeros(3)).check()
    import ctypes as C
    from bipymc_amd import _lib as L
    lib = L.load()
    log = C.create_string_buffer(256)
    assert lib.bpm_check_pointwise(WC.SOURCES[1].encode(), 65, None, log, len(log)) != 0
    assert b"bpm_check_pointwise: w must be 1 ... 64 (got 65)" in lib.bpm_last_error()


@pytest.fixture(scope="module")
def case():
    H = WC.make_history(9, 12, 4)
    pw = WC.pointwise(3, WC.make_data(11, 3))
    return H, pw


@pytest.mark.parametrize("n_burn", [0, 12 * 2 + 5, 12 * 9 - 1])
def test_one_and_three_unequal_ranks_stay_within_the_bound_and_agree_with_themselves(case, n_burn):
    H, pw = case
    L = pw(H.reshape(-1, H.shape[2])[n_burn:])
    ref = None
    for shares in ([12], [5, 3, 4]):
        fr = FakePointwiseRanks(H, shares)
        res = PW.compute(fr.pointwise, lambda x: x, pw, n_burn, fr.N, fr.G)
        assert isinstance(res, PosteriorWaic) and res.values is None
        rows = max(int(p[2]) for p in fr.pointwise(pw, n_burn, False))
        ref = WC.check_result(res, L, rows, 1, len(shares), ref=ref, what="shares %r, n_burn %d" % (shares, n_burn))
        # "all ranks return identical bits": every rank runs compute on the same gathered parts
        WC.same_result(res, PW.compute(fr.pointwise, lambda x: [np.copy(a) if isinstance(a, np.ndarray) else a for a in x], pw, n_burn, fr.N, fr.G))
    fr = FakePointwiseRanks(H, [4, 4, 4])                # equal shares: the values come back in super-chain order
    res = PW.compute(fr.pointwise, lambda x: x, pw, n_burn, fr.N, fr.G, values=True)
    WC.bits_equal(res.values, L)
    WC.check_result(res, L, max(int(p[2]) for p in fr.pointwise(pw, n_burn, False)), 1, 3, ref=ref, what="equal shares with values")


def test_merge_formulas_on_empty_parts_and_values_that_are_not_finite():
    inf = np.inf
    # per datum (columns): both sides hold values | a empty | b empty | both empty | equal maxima | far apart (the smaller side underflows)
    a = (np.array([3, 0, 2, 0, 1, 5]), np.array([1.0, -inf, -2.0, np.nan, 7.0, 800.0]), np.array([2.5, 0.0, 1.5, np.nan, 1.0, 4.0]))
    b = (np.array([2, 4, 0, 0, 1, 3]), np.array([4.0, 0.5, inf, -inf, 7.0, -900.0]), np.array([1.25, 3.0, np.nan, 0.0, 1.0, 2.0]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # no inf - inf, no NaN is formed on the way
        n, m, s = PW.merge_lse([a, b])
        n3, m3, s3 = PW.merge_lse([b, (np.zeros(6, dtype=np.int64), np.full(6, np.nan), np.full(6, np.nan)), a])
    assert n.tolist() == n3.tolist() == [5, 4, 2, 0, 2, 8]
    assert m.tolist() == m3.tolist() == [4.0, 0.5, -2.0, -inf, 7.0, 800.0]
    want = [2.5 * np.exp(-3.0) + 1.25, 3.0, 1.5, 0.0, 2.0, 4.0]
    assert np.allclose(s, want, rtol=4 * WC.U, atol=0.0) and np.allclose(s3, want, rtol=4 * WC.U, atol=0.0)
    assert s[1] == 3.0 and s[2] == 1.5 and s[3] == 0.0 and s[5] == 4.0      # untouched sides are copied, not recomputed
    # the finish: one datum of every kind
    counts = (np.array([4, 3, 0, 3, 3, 2]), np.array([0, 0, 0, 0, 1, 1]), np.array([0, 0, 0, 1, 0, 1]), np.array([0, 1, 4, 0, 0, 0]))
    res = PW.finish_waic(counts, np.zeros(6), np.full(6, 2.0), np.zeros(6), np.full(6, 8.0), 4)
    assert res.lppd_i[0] == np.log(2.0) - np.log(4.0) and res.p_waic_i[0] == 2.0 and res.mean_i[0] == 0.0
    assert res.lppd_i[1] == res.lppd_i[0] and np.isnan(res.p_waic_i[1]) and res.mean_i[1] == -inf          # some -inf
    assert res.lppd_i[2] == -inf and np.isnan(res.p_waic_i[2]) and res.mean_i[2] == -inf                    # all -inf
    assert res.lppd_i[3] == inf and np.isnan(res.p_waic_i[3]) and res.mean_i[3] == inf                      # a +inf
    assert np.isnan([res.lppd_i[4], res.p_waic_i[4], res.mean_i[4], res.lppd_i[5], res.mean_i[5]]).all()    # a NaN (with a +inf too)
    assert np.isnan(res.elpd_waic) and np.isnan(res.se) and res.n_high_var == 1


def test_rules_for_values_that_are_not_finite_are_scipys_and_numpys_column_by_column():
    H = WC.make_history(6, 8, 4, seed=3)
    Y = WC.make_data(9, 4)
    rows = H.reshape(-1, 4)
    Y[1, 2], Y[1, 3] = rows[5, 2], 1.0                   # one -inf
    Y[2, 3] = np.inf                                     # all -inf
    Y[3, 2], Y[3, 3] = rows[17, 2], -1.0                 # one +inf
    Y[4, 2], Y[4, 3] = rows[30, 2], 0.0                  # one NaN (0 / 0)
    Y[5, 3] = np.nan                                     # all NaN
    Y[6, 3] = -np.inf                                    # all +inf
    pw = WC.pointwise(4, Y)
    L = pw(rows)
    assert (L[:, 1] == -np.inf).sum() == 1 and (L[:, 2] == -np.inf).all() and (L[:, 3] == np.inf).sum() == 1 and np.isnan(L[:, 4]).sum() == 1
    for shares in ([8], [3, 1, 4]):
        fr = FakePointwiseRanks(H, shares)
        res = PW.compute(fr.pointwise, lambda x: x, pw, 0, fr.N, fr.G)
        WC.check_result(res, L, len(rows), 1, len(shares), what="not finite, shares %r" % (shares,))
        assert np.isfinite(res.lppd_i[1]) and res.lppd_i[2] == -np.inf and res.lppd_i[3] == np.inf and np.isnan(res.lppd_i[4])
        assert res.n_neg_inf.tolist() == [0, 1, 48, 0, 0, 0, 0, 0, 0] and res.n_pos_inf.tolist() == [0, 0, 0, 1, 0, 0, 48, 0, 0]
        assert res.n_nan.tolist() == [0, 0, 0, 0, 1, 48, 0, 0, 0]
        clean = PW.compute(fr.pointwise, lambda x: x, WC.pointwise(4, WC.make_data(9, 4)), 0, fr.N, fr.G)
        WC.same_result(res, clean, "the other data", skip=[1, 2, 3, 4, 5, 6])


def test_errors_are_worded_as_the_other_statistics_word_them(case):
    H, pw = case
    fr = FakePointwiseRanks(H, [6, 6])

    def run(pw=pw, n_burn=0, **kw):
        return PW.compute(fr.pointwise, lambda x: x, pw, n_burn, fr.N, fr.G, **kw)

    with pytest.raises(TypeError, match="param_est_waic: pw must be a HipPointwise"):
        run(pw=lambda x: x)
    with pytest.raises(ValueError, match=r"param_est_waic: n_burn must be >= 0 \(got -1\)"):
        run(n_burn=-1)
    with pytest.raises(ValueError, match=r"param_est_waic: the window is empty \(n_burn = 108 is at or beyond the last super-chain row\)"):
        run(n_burn=12 * 9)
    assert run(n_burn=12 * 9 - 1).n == 1
    fr.G = 10
    with pytest.raises(RuntimeError, match="the ranks hold 108 rows of the window"):
        run()
    from bipymc_amd.samplers import DeMc
    with pytest.raises(RuntimeError, match="param_est_waic: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).param_est_waic(pw)


def test_compare_waic_se_and_str_against_numpy_one_liners(case):
    H, pw = case
    fr = FakePointwiseRanks(H, [12])
    a = PW.compute(fr.pointwise, lambda x: x, pw, 12, fr.N, fr.G)
    b = PW.compute(fr.pointwise, lambda x: x, WC.pointwise(3, pw.data, params=[0.25, 0.5, 0.002]), 12, fr.N, fr.G)
    nd = pw.n_data
    assert a.se == np.sqrt(nd * np.var(a.elpd_i)) and a.waic == -2.0 * a.elpd_waic and a.elpd_waic == np.sum(a.lppd_i - a.p_waic_i)
    diff, se = compare_waic(a, b)
    assert diff == a.elpd_waic - b.elpd_waic and se == np.sqrt(nd * np.var(a.elpd_i - b.elpd_i))
    assert compare_waic(b, a) == (-diff, se) and compare_waic(a, a) == (0.0, 0.0)
    text = str(a)
    for want in ("elpd_waic", "%.6g" % a.elpd_waic, "%.6g" % a.se, "%.6g" % a.p_waic, "p_waic_i > 0.4", "%d" % a.n):
        assert want in text, (want, text)
    with pytest.raises(ValueError, match="over 11 and 4 data points"):
        compare_waic(a, PW.compute(fr.pointwise, lambda x: x, WC.pointwise(3, pw.data[:4]), 12, fr.N, fr.G))
    with pytest.raises(ValueError, match="over 96 and 108 draws"):
        compare_waic(a, PW.compute(fr.pointwise, lambda x: x, pw, 0, fr.N, fr.G))
    with pytest.raises(TypeError, match="must be PosteriorWaic"):
        compare_waic(a, 3.0)


def test_host_side_merge_and_layout_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/pointwise_host_main.cpp: pointwise.h's layout arithmetic and pointwise_rows.h's merge in a plain C++ program of their own"""
    exe = str(tmp_path / "pointwise_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "bipymc_amd", "csrc"), os.path.join(HERE, "pointwise_host_main.cpp"), "-o", exe, "-ldl"])
    out = subprocess.check_output([exe]).decode()
    print(out)
    f = dict(line.split(None, 1) for line in out.splitlines() if line and not line.startswith("#"))
    assert int(f["layouts"]) > 10000 and int(f["layout_violations"]) == 0
    assert int(f["merges"]) >= 300 and int(f["merge_violations"]) == 0
    # the C entry point gives the same layout
    import ctypes as C
    from bipymc_amd import _lib as L
    lib = L.load()
    lay = (C.c_int64 * 4)()
    assert lib.bpm_pointwise_layout(3, 1, 2050, 200, lay) == 0
    assert list(lay) == [int(x) for x in f["layout_3_2050_200"].split()]
