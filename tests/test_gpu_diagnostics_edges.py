"""The four kernels of bipymc_amd/csrc/diagnostics.h at the shapes where their tiling changes, on badly conditioned columns and on histories
with a non-finite value: what bpm_diag_split_moments / bpm_diag_autocov return -- mean_of_means, m2_of_means, sum_of_vars and the lag sums --
element by element against the exactly rounded reference of tests/_diag_exact.py, inside the bound derived there and nothing else.

The constants the shapes are chosen around (diagnostics.h, bpm_diag_autocov): DIAG_UNR = 8 loads per batch of the split pass, DIAG_B = 8 rows
per batch and DIAG_T = 16 lags per launch of the autocovariance pass; ld = d rounded up to even, kw = min(ld, 256) columns per tile,
cpw = 256 // kw chains side by side in a workgroup, n_groups = ceil(n_local / cpw) column groups of which nb = min(n_groups, 384 // n_kt)
workgroups walk one or more.

Columns, by k % 8 (edge_history): unit normal; the same at offset 1e8; denormals (1e-310); constant within every half-chain (sum_of_vars
and every lag sum are EXACTLY 0); constant in all chains but one; a step of 1e6 between the two halves; scale 1e3; a random walk.

Column isolation (test_a_non_finite_value_stays_in_its_coordinate): one NaN / +inf / -inf in the first half, the second half or the dropped
middle row.  The poisoned coordinate's raw outputs are NaN (untouched for the dropped row), every other coordinate's raw outputs, r_hat, ess,
tau and lags_used are the bits of the clean run on the same handle.  Before the idle lanes of diag_autocov_kernel were given a zero ring the
(chain 0, coordinate 0) cases failed at every shape here (n_local % cpw != 0: an idle lane multiplied 0 by column 0's NaN and its workgroup
summed that into every coordinate); before diag_split_moments_kernel stopped clamping with fmax, a poisoned coordinate's sum_of_vars was
finite (fmax(NaN, 0) = 0).

MEASURED on an MI355X, largest |device - exact| / bound over this file (test_zz_worst_ratios prints them):
    mean_of_means 0.333   m2_of_means 0.165   sum_of_vars 0.153   lag sums 0.215
(all four at N = 4, d = 513, n = 4, where a sum has the fewest terms and the worst-case bound the least slack; at N = 200, d = 257 the
largest is 0.026.  The float64 kernel-order model of tests/test_diag_exact_host.py gives the same four figures on the same histories.)

End to end (test_smallest_windows_end_to_end): diagnostics.compute against reference() of tests/test_diagnostics_host.py under _check of
tests/test_gpu_diagnostics.py at n = 4, 5, 8.  The seeds (E2E_CASES) were chosen on the CPU so that the reference alone leaves
margin > 1e-6 on every coordinate: _check's allowance is not used, the test asserts that none is excluded."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _diag_exact as DX  # noqa: E402
from _history_cases import _engine  # noqa: E402
from test_diagnostics_host import _ar1, reference  # noqa: E402
from test_gpu_diagnostics import _check, _device  # noqa: E402

WORST = dict((key, 0.0) for key in DX.KEYS)


def edge_history(rows, N, d, g0, seed):
    """(rows, N, d) with the window [g0, rows); the column kinds of the module docstring"""
    rs = np.random.RandomState(seed)
    X = rs.normal(size=(rows, N, d))
    n = (rows - g0) // 2
    second = np.arange(rows) >= rows - n
    for k in range(d):
        kind = k % 8
        if kind == 1:
            X[:, :, k] += 1e8
        elif kind == 2:
            X[:, :, k] *= 1e-310
        elif kind == 3:
            level = rs.normal(size=(2, N))
            X[:, :, k] = level[second.astype(int)]
        elif kind == 4:
            X[:, :, k] = 1.25
            X[:, N // 2, k] = rs.normal(size=rows)
        elif kind == 5:
            X[second, :, k] += 1e6
        elif kind == 6:
            X[:, :, k] *= 1e3
        elif kind == 7:
            X[:, :, k] = np.cumsum(X[:, :, k], axis=0)
    return X


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _raw(e, g0, g1):
    """every raw output of the two entry points over the window: dict over DX.KEYS (c: all n lags)"""
    mean, m2, sv, m, n = e.diag_split_moments(g0, g1)
    return dict(mean=mean, m2=m2, sum_var=sv, c=e.diag_autocov(0, n), m=m, n=n)


def _lag_requests(n):
    req = [(0, 1), (0, n), (n - 1, 1)]
    if n == 33:
        req += [(16, 16), (16, 17), (32, 1)]
    if n == 20:
        req += [(16, 4)]                       # a last launch with fewer than DIAG_T live lags
    return req


def _compare(N, d, rows, g0, seed):
    from bipymc_amd import _lib as L
    X = edge_history(rows, N, d, g0, seed)
    ref, bnd = DX.exact(X, g0, rows), DX.bound(X, g0, rows)
    n = ref["n"]
    e = _engine(N, d)
    try:
        e.set_history(X, X[-1])
        mean, m2, sv, m, n_dev = e.diag_split_moments(g0, rows)
        assert (m, n_dev) == (2 * N, n)
        got = dict(mean=mean, m2=m2, sum_var=sv)
        for t0, n_lags in _lag_requests(n):
            got["c"] = e.diag_autocov(t0, n_lags)
            assert got["c"].shape == (n_lags, d)
            sl = slice(t0, t0 + n_lags)
            worst = DX.worst_ratios(got, dict(ref, c=ref["c"][sl]), dict(bnd, c=bnd["c"][sl]))
            print("N %d d %d n %d g0 %d lags [%d, %d): error / bound %s" % (N, d, n, g0, t0, t0 + n_lags,
                                                                            ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
            for key in DX.KEYS:
                WORST[key] = max(WORST[key], worst[key])
            assert max(worst.values()) <= 1.0, (t0, n_lags, worst)
            flat = [k for k in range(d) if k % 8 == 3]          # constant within every half-chain: exactly zero
            assert np.all(got["sum_var"][flat] == 0.0) and np.all(got["c"][:, flat] == 0.0)
        with pytest.raises(L.BpmError, match=r"must lie in \[0, n\)"):
            e.diag_autocov(n - 1, 2)
        with pytest.raises(L.BpmError, match=r"must lie in \[0, n\)"):
            e.diag_autocov(0, n + 1)
    finally:
        e.close()


# draws per half-chain: 4 = the minimum; 7 / 8 / 9 around DIAG_UNR and DIAG_B; 15 / 16 / 17 around DIAG_T (17: a second launch of one lag);
# 20: a last launch of 4 lags; 31 / 33 around two launches.  (rows, g0): odd windows drop their middle row, g0 > 0 moves both halves.
# N = 10, d = 6: ld = 6, cpw = 42, one ragged group, the six kinds of column that are not plain.
@pytest.mark.parametrize("n,rows,g0", [(4, 8, 0), (5, 12, 1), (7, 14, 0), (8, 19, 2), (9, 18, 0), (15, 33, 2), (16, 32, 0), (17, 35, 0),
                                       (20, 40, 0), (31, 64, 2), (33, 70, 3)])
def test_draws_per_half_chain(n, rows, g0):
    assert (rows - g0) // 2 == n
    _compare(10, 6, rows, g0, seed=100 + n)


# row width and chains against cpw; n = 4 (rows 9: odd) or 5 (rows 11, g0 = 1), and n = 17 where two tiles meet two launches
@pytest.mark.parametrize("N,d,rows,g0", [
    (129, 1, 9, 0),          # ld 2, cpw 128: n_local % cpw = 1
    (128, 2, 11, 1),         # n_local % cpw = 0
    (127, 2, 9, 0),          # ... = cpw - 1, n_local < cpw
    (200, 2, 11, 1),         # two groups, the second partial (72 of 128)
    (4, 3, 9, 0),            # ld 4, cpw 64: n_local < cpw
    (10, 3, 11, 1),
    (63, 3, 9, 0),           # cpw - 1
    (64, 3, 11, 1),          # 0
    (65, 3, 9, 0),           # 1
    (43, 5, 11, 1),          # ld 6, cpw 42: 1
    (7, 100, 9, 0),          # cpw 2: 1 = cpw - 1
    (8, 100, 11, 1),         # 0
    (5, 127, 9, 0),          # ld 128, cpw 2
    (6, 128, 11, 1),
    (4, 129, 9, 0),          # ld 130: cpw 1, 126 lanes of the workgroup idle
    (5, 255, 11, 1),         # ld 256
    (5, 256, 9, 0),
    (5, 257, 35, 0),         # ld 258: two column tiles, the second holding two columns; n = 17: two launches
    (200, 257, 9, 0),        # n_groups = 200 > 384 / n_kt = 192: eight workgroups walk a second group
    (4, 300, 11, 1),
    (4, 513, 9, 0),          # three tiles
])
def test_row_width_and_chains_against_the_tile(N, d, rows, g0):
    _compare(N, d, rows, g0, seed=1000 + N + d)


# ---- column isolation ----------------------------------------------------------------------------------------------------------------------
ISO_ROWS = 13                   # n = 6: first half rows 0 ... 5, row 6 dropped, second half rows 7 ... 12 (row 12 is the state: never poisoned)
ISO_SHAPES = [(10, 3), (7, 100), (200, 2)]      # cpw 64 with a ragged only group; cpw 2 and an odd N; cpw 128, two groups


def _positions(N, d):
    return [(0, 0), (0, d - 1), (N - 1, 0), (1, 1)]


@pytest.mark.parametrize("pos", range(4))
@pytest.mark.parametrize("N,d", ISO_SHAPES)
def test_a_non_finite_value_stays_in_its_coordinate(N, d, pos):
    chain, coord = _positions(N, d)[pos]
    X = _ar1(ISO_ROWS, N, np.linspace(0.0, 0.6, d), seed=7 + N)
    others = [k for k in range(d) if k != coord]
    e = _engine(N, d)
    try:
        e.set_history(X, X[-1])
        clean, clean_fin = _raw(e, 0, ISO_ROWS), _device(e)
        assert clean["n"] == 6 and np.isfinite(clean_fin.ess).all()
        for value in (np.nan, np.inf, -np.inf):
            for row in (3, 6, 9):
                Y = X.copy()
                Y[row, chain, coord] = value
                e.set_history(Y, Y[-1])
                raw, fin = _raw(e, 0, ISO_ROWS), _device(e)
                what = "%r at row %d, chain %d, coordinate %d" % (value, row, chain, coord)
                for key in DX.KEYS:
                    assert np.array_equal(_bits(raw[key][..., others]), _bits(clean[key][..., others])), \
                        "%s changed %s of other coordinates: %s -> %s" % (what, key, clean[key][..., others], raw[key][..., others])
                for f in ("r_hat", "ess", "tau", "lags_used"):
                    assert np.array_equal(_bits(getattr(fin, f)[others]), _bits(getattr(clean_fin, f)[others])), (what, f)
                for key in DX.KEYS:
                    if row == 6:
                        assert np.array_equal(_bits(raw[key][..., coord]), _bits(clean[key][..., coord])), (what, key)
                    else:
                        assert np.isnan(raw[key][..., coord]).all(), "%s: %s of its own coordinate is %s" % (what, key, raw[key][..., coord])
                if row != 6:
                    assert np.isnan(fin.r_hat[coord]) and np.isnan(fin.ess[coord]) and np.isnan(fin.tau[coord]), what
    finally:
        e.close()


# ---- end to end at the smallest windows -------------------------------------------------------------------------------------------------------
E2E_PHIS = [0.0, 0.5, 0.9, 0.5, 0.0]
E2E_CASES = [(4, 9, 0, 11), (5, 12, 2, 12), (8, 16, 0, 13), (8, 19, 2, 14)]      # (n, rows, g0, seed)


@pytest.mark.parametrize("n,rows,g0,seed", E2E_CASES)
def test_smallest_windows_end_to_end(n, rows, g0, seed):
    X = _ar1(rows, 10, E2E_PHIS, seed=seed)
    ref = reference(X, g0=g0)
    assert ref["n"] == n and np.isfinite(ref["ess"]).all()
    assert (ref["margin"] > 1e-6).all(), ref["margin"]          # nothing for _check to exclude
    e = _engine(10, 5)
    try:
        e.set_history(X, X[-1])
        got = _device(e, g0=g0)
    finally:
        e.close()
    assert got.n_draws == n and got.n_half_chains == 20 and got.window == (g0, rows)
    _check(got, ref)
    np.testing.assert_allclose(got.ess, ref["ess"], rtol=1e-8)


def test_zz_worst_ratios():
    """(last in the file: what the tests above saw)"""
    print("largest |device - exact| / bound: " + ", ".join("%s %.3g" % (key, WORST[key]) for key in DX.KEYS))
    assert all(0.0 <= v <= 1.0 for v in WORST.values())
