"""tests/_diag_exact.py without a GPU: the exact statement of bpm_diag_split_moments / bpm_diag_autocov against the definitions written out in
fractions.Fraction, against BlockParts of tests/test_diagnostics_host.py and against a float64 evaluation in the kernels' order
(bipymc_amd/csrc/diagnostics.h) inside the derived bound; how the bound scales with a column's offset; non-finite values.
No tolerance appears here but _diag_exact.bound()."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _diag_exact as DX  # noqa: E402
from test_diagnostics_host import BlockParts, _ar1  # noqa: E402


def kernel_order_model(H, g0, g1, shifted=True):
    """float64, operation by operation in the kernels' order: the half's first value as the shift, sequential sums over the rows, M2 = sb - sa m0
    clamped at 0, the 256-lane tree of diag_means_final_kernel, the lag products accumulated row by row and half-chain by half-chain (the
    products rounded: NumPy has no fma).  shifted=False: the textbook one-pass sums without the shift -- what the bound must NOT let through."""
    h = DX.halves(H, g0, g1)
    n, m, d = h.shape
    sh = h[0] if shifted else np.zeros_like(h[0])
    sa, sb = np.zeros((m, d)), np.zeros((m, d))
    for i in range(n):
        dd = h[i] - sh
        sa = sa + dd
        sb = sb + dd * dd
    m0 = sa * (1.0 / n)
    v = sb - sa * m0
    mean = np.where(v == v, sh + m0, np.nan)         # (a half-chain with a non-finite value: M2 = NaN and, with it, the mean)
    M2 = np.where(v < 0.0, 0.0, v)

    def tree(a):                                     # (m, d) -> (d,): lane j % 256 adds its rows in order, then halving steps
        lanes = np.zeros((256, d))
        for j in range(m):
            lanes[j % 256] = lanes[j % 256] + a[j]
        o = 128
        while o > 0:
            lanes[:o] = lanes[:o] + lanes[o:2 * o]
            o //= 2
        return lanes[0]

    mu = tree(mean) / m
    e = mean - mu
    out = dict(mean=mu, m2=tree(e * e), sum_var=tree(M2 / (n - 1.0)))
    y = h - mean
    c = np.zeros((n, d))
    for t in range(n):
        acc = np.zeros(d)
        for j in range(m):
            for i in range(t, n):
                acc = acc + y[i, j] * y[i - t, j]
        c[t] = acc / n
    out["c"] = c
    return out


def _fraction_definitions(H, g0, g1):
    """the definitions, one Fraction at a time (tiny shapes only)"""
    h = DX.halves(H, g0, g1)
    n, m, d = h.shape
    out = dict(mean=np.empty(d), m2=np.empty(d), sum_var=np.empty(d), c=np.empty((n, d)))
    for k in range(d):
        x = [[Fraction(float(h[i, j, k])) for i in range(n)] for j in range(m)]
        xbar = [sum(r) / n for r in x]
        y = [[v - b for v in r] for r, b in zip(x, xbar)]
        mu = sum(xbar) / m
        out["mean"][k] = float(mu)
        out["m2"][k] = float(sum((b - mu) ** 2 for b in xbar))
        out["sum_var"][k] = float(sum(sum(v * v for v in r) / (n - 1) for r in y))
        for t in range(n):
            out["c"][t, k] = float(sum(sum(r[i] * r[i + t] for i in range(n - t)) / n for r in y))
    return out


def _edge_block(rows, N, seed):
    """columns: unit normal, offset 1e8 with unit spread, denormals, constant in every half-chain, a large step between the halves"""
    rs = np.random.RandomState(seed)
    X = rs.normal(size=(rows, N, 5))
    X[:, :, 1] += 1e8
    X[:, :, 2] *= 1e-310
    X[:, :, 3] = 2.5
    X[rows // 2 + 1:, :, 4] += 1e6
    return X


@pytest.mark.parametrize("g0,g1", [(0, 11), (1, 11), (2, 10)])
def test_integer_scheme_equals_the_definitions_in_fractions(g0, g1):
    X = _edge_block(11, 3, seed=1)
    got, want = DX.exact(X, g0, g1), _fraction_definitions(X, g0, g1)
    for key in DX.KEYS:
        assert np.array_equal(got[key], want[key]), key                 # both are the correctly rounded value: the same bits
    assert got["n"] == (g1 - g0) // 2 and got["m"] == 6
    assert got["sum_var"][3] == 0.0 and np.all(got["c"][:, 3] == 0.0) and got["m2"][3] == 0.0
    assert got["mean"][2] != 0.0 and abs(got["mean"][2]) < 1e-309       # the denormal column's mean is itself a denormal


@pytest.mark.parametrize("rows,N", [(61, 16), (40, 7)])
def test_blockparts_lies_inside_the_bound_on_well_conditioned_data(rows, N):
    X = _ar1(rows, N, [0.0, 0.5, 0.9, -0.2], seed=3)
    X[:, :N // 2, 3] += 1.5
    ref, bnd = DX.exact(X, 1, rows), DX.bound(X, 1, rows)
    bp = BlockParts(X)
    mu, m2, sv, m, n = bp.split(1, rows)
    assert (m, n) == (ref["m"], ref["n"])
    worst = DX.worst_ratios(dict(mean=mu, m2=m2, sum_var=sv, c=bp.autocov(0, n)), ref, bnd)
    print("BlockParts against the exact reference, error / bound:", worst)
    assert max(worst.values()) <= 1.0, worst
    # the bound is a rounding bound, not a tolerance: a relative 1e-12 on either quantity is outside it (gamma_{m n} = 1e-13 here)
    assert np.all(bnd["sum_var"] < 1e-12 * ref["sum_var"]) and np.all(bnd["c"][0] < 1e-12 * ref["c"][0])


def test_kernel_order_evaluation_lies_inside_the_bound_and_the_bound_scales_as_derived():
    rows, N = 35, 10                                  # n = 17
    X = _edge_block(rows, N, seed=7)
    ref, bnd = DX.exact(X, 0, rows), DX.bound(X, 0, rows)
    n, m = ref["n"], ref["m"]
    worst = DX.worst_ratios(kernel_order_model(X, 0, rows), ref, bnd)
    print("kernel-order float64 against the exact reference, error / bound:", worst)
    assert max(worst.values()) <= 1.0, worst
    # column 1 is column 0's kind of data at offset 1e8.  delta = u |mean| dominates its half-chain means, and the m of them are added
    # unshifted: (m + 1) u |mean| for the mean of the means
    delta = DX.U * 1e8
    assert (m + 1) * delta <= bnd["mean"][1] <= (m + 1.01) * delta
    # ... the shift keeps the variances free of the offset (the data are quantised to 2^-26 there, the bound is not)
    assert bnd["sum_var"][1] < 4 * bnd["sum_var"][0] * ref["sum_var"][1] / ref["sum_var"][0]
    # ... c[0] moves by delta^2 only, c[t >= 1] by 2 t delta max|y| / n per half-chain: linear in t and in the offset
    assert bnd["c"][0, 1] < 1e-3 * bnd["c"][1, 1]
    ymax = np.abs(DX.halves(X, 0, rows)[:, :, 1] - 1e8).max()
    for t in (1, 2, 8, n - 1):
        lead = 2 * t * delta * ymax * m / n
        assert 0.25 * lead <= bnd["c"][t, 1] <= 1.1 * lead, t          # (every half-chain's max |y| is above a quarter of the largest)
    assert bnd["c"][1, 0] < 1e-4 * bnd["c"][1, 1]                      # without the offset the same lag is held four digits closer
    # the textbook sums without the shift lose the variance at offset 1e8: the bound does not let them through
    naive = kernel_order_model(X, 0, rows, shifted=False)
    assert abs(naive["sum_var"][1] - ref["sum_var"][1]) > 100 * bnd["sum_var"][1]
    # exactly zero where the definitions are exactly zero
    got = kernel_order_model(X, 0, rows)
    assert got["sum_var"][3] == 0.0 and np.all(got["c"][:, 3] == 0.0)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("row", [1, 4, 5, 8])       # first half, its last row, the dropped middle row, second half
def test_non_finite_values_stay_in_their_coordinate(value, row):
    X = _ar1(11, 5, [0.3, 0.5, 0.0], seed=5)
    clean = DX.exact(X, 0, 11)
    Y = X.copy()
    Y[row, 2, 1] = value
    got, bnd = DX.exact(Y, 0, 11), DX.bound(Y, 0, 11)
    for key in DX.KEYS:
        hit = row != 5
        assert np.isnan(got[key][..., 1]).all() == hit and np.isnan(bnd[key][..., 1]).all() == hit, key
        keep = [0, 2] if hit else [0, 1, 2]
        assert np.array_equal(got[key][..., keep], clean[key][..., keep]), key


def test_too_short_a_window_is_an_error():
    with pytest.raises(ValueError, match="at least 4"):
        DX.exact(np.zeros((7, 2, 2)), 0, 7)
