"""What tests/test_waic_host.py and tests/test_gpu_waic.py share: the pointwise functions of the cases (HIP source and the same statement in
NumPy), the exact reference, the bounds with their derivation, and the checker.

THE FUNCTIONS are built from + - * / only, each operation written once in the same association on both sides; the source is compiled
-ffp-contract=off, so the (rows, n_data) matrix of the device (values=True) equals python_fn's bit for bit, and that matrix -- not a second
evaluation -- is what every reduction is compared with.  Every function uses the datum's index i and its own values y, and reads x[d - 1]:
a shifted or shared datum, or a row cut short, shows in the values.  With w = 4 the term - y[3] / ((y[2] - x[2])^2) plants what is not
finite in ONE datum: y[2] equal to a row's x[2] gives -inf (y[3] = 1), +inf (y[3] = -1) or NaN (y[3] = 0, 0 / 0) at exactly that row, an
infinite or NaN y[3] at every row; all other data have y[3] = 0 and a y[2] no row holds.

THE REFERENCE.  Per datum, over the column l of that matrix: lppd = log(sum exp(l)) - log(n) in mpmath at 200 bits (the inputs are the
float64 values themselves, so the result is exact to far below the bounds); mean and variance in np.longdouble, as tests/test_derived_host.py
computes them.  A column with a value that is not finite is compared with scipy.special.logsumexp / np.var / np.mean for equality instead.

THE BOUNDS.  u = 2^-53.
  lppd_i.  The device keeps (m, s), s = sum exp(l - m) with m the running maximum, so s >= 1 and every term is <= 1 (pointwise_rows.h).  Let
  E bound the error of the device's exp in ulps.  A row that does not raise the maximum adds t = exp(a), a = l - m <= 0: the subtraction's
  rounding moves t by |a| exp(a) u <= u / e, the exp by E u, the addition rounds s by u: at most (E + 2) u relative to s, since s >= 1.  A
  row that raises it forms s exp(a) + 1: one exp, one product, one sum -- (E + 2) u again, but the argument's rounding now scales all of s:
  |a| s exp(a) / (s exp(a) + 1) u.  That factor exceeds 1 only where s exp(a) is of order one or more with |a| > 1, i.e. s >~ e^|a| / |a| rows
  of the part lie behind it, so over a part its sum stays below the part's rows: it is paid from E, which is TWICE the largest error seen
  (below), i.e. from >= E / 2 u per row.  A part of r rows therefore ends with s off by <= r (E + 2) u relatively; folding P parts and then
  K ranks costs two exps, two products and a sum per merge, of which one exp is exp(0) = 1: <= (E + 2) u each.  log(s) turns a relative
  error into an absolute one and adds its own rounding (the host's log, <= 1 ulp of a value <= log(n) <= r + P + K), and m + log(s) and the
  subtraction of log(n) round once each, one of them relative to lppd itself, the other to a value off it by log(n) <= r + P + K:
      |lppd_i - exact| <= ((r + P + K) (E + 2) + E + 2) u + u |lppd_i|.
  mean_i, p_waic_i: trace_acc.h's sums merged in a fixed order -- tests/test_traces_host.py: trace_bound(n, max |l|, max |l - mean|), derived
  there for any summation order and any number of merges.
  E: no accuracy table of the HIP math functions lies under the ROCm installation's documentation, so it is measured, with code that knows
  nothing of the pointwise kernel (tools/waic_bound.py: a HipFunction returning exp and log through param_est_fn(values=True), against
  mpmath; profiles/waic_bound.txt).  Largest error seen: E_SEEN ulp; E = 2 E_SEEN rounded up, since a finite sample cannot show the worst case.
No tolerance was tuned on the pointwise kernel's output."""
import warnings

import numpy as np

from test_traces_host import trace_bound

U = 2.0 ** -53
E_SEEN = 0.8368       # profiles/waic_bound.txt: the largest error of the device's exp (0.8368) / log (0.6235) over 65536 arguments each, in ulps
E = 2                 # twice that, rounded up to a whole ulp

PARAMS = [0.75, 0.5, 0.001]

_HEAD = "__device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p) {\n"
SOURCES = {
    1: _HEAD + "    const double r = y[0] - x[0];\n    return -0.5 * r * r * p[0] + x[d - 1] * p[1] - i * p[2];\n}",
    3: _HEAD + "    const double r = y[1] - (x[0] + x[1] * y[0]);\n    return -0.5 * r * r * p[0] + x[d - 1] * y[2] - i * p[2];\n}",
    4: _HEAD + "    const double r = y[1] - (x[0] + x[1] * y[0]);\n    const double t = y[2] - x[2];\n"
               "    return -0.5 * r * r * p[0] + x[d - 1] * p[1] - i * p[2] - y[3] / (t * t);\n}",
    9: _HEAD + "    const double r = y[1] - (x[0] + x[1] * y[0]);\n    return -0.5 * r * r * p[0] + x[d - 1] * y[8] - i * p[2];\n}",
}


def _python_fn(w):
    def fn(X, Y, p):
        X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        i = np.arange(len(Y), dtype=np.float64)[None, :]
        x0, x1, xl = X[:, 0:1], X[:, 1:2], X[:, -1:]
        with np.errstate(all="ignore"):
            if w == 1:
                r = Y[None, :, 0] - x0
                return -0.5 * r * r * p[0] + xl * p[1] - i * p[2]
            r = Y[None, :, 1] - (x0 + x1 * Y[None, :, 0])
            if w == 4:
                t = Y[None, :, 2] - X[:, 2:3]
                return -0.5 * r * r * p[0] + xl * p[1] - i * p[2] - Y[None, :, 3] / (t * t)
            return -0.5 * r * r * p[0] + xl * Y[None, :, w - 1] - i * p[2]
    return fn


def make_data(n_data, w, seed=0):
    """(n_data, w): abscissae in [0, 1], ordinates near the line 1 + 2 t; w = 4: column 2 a selector no row of make_history holds (100 + i),
    column 3 zero"""
    rs = np.random.RandomState(1000 + 7 * n_data + w + seed)
    Y = rs.normal(size=(n_data, w))
    if w > 1:
        Y[:, 0] = rs.uniform(0.0, 1.0, size=n_data)
        Y[:, 1] = 1.0 + 2.0 * Y[:, 0] + 0.3 * rs.normal(size=n_data)
    if w == 4:
        Y[:, 2] = 100.0 + np.arange(n_data)
        Y[:, 3] = 0.0
    return Y


def pointwise(w, data, params=PARAMS):
    from bipymc_amd import HipPointwise
    return HipPointwise(SOURCES[w], data=data, params=params, python_fn=_python_fn(w))


def make_history(G, N, d, seed=0):
    """(G, N, d): a posterior-like cloud about the line's parameters (1, 2), every value distinct"""
    rs = np.random.RandomState(50 + seed)
    X = rs.normal(size=(G, N, d)) * 0.2
    X[:, :, 0] += 1.0
    X[:, :, 1] += 2.0
    return X


def lppd_bound(rows_per_part, parts, ranks, lppd):
    return ((rows_per_part + parts + ranks) * (E + 2) + E + 2) * U + U * abs(lppd)


def exact_lppd(col, n=None):
    """log(sum exp(col)) - log(n) (n: len(col)) of a finite float64 column, exactly rounded (mpmath, 200 bits) -> mpf"""
    import mpmath as mp
    with mp.workprec(200):
        top = mp.mpf(float(np.max(col)))
        tot = mp.fsum(mp.exp(mp.mpf(float(v)) - top) for v in col)
        return top + mp.log(tot) - mp.log(len(col) if n is None else n)


def abs_error(got, exact):
    """|got - exact| for a float64 and an mpf, formed at the reference's precision"""
    import mpmath as mp
    with mp.workprec(200):
        return float(abs(mp.mpf(float(got)) - exact))


def reference(L):
    """per column of the matrix L (rows, n_data): None where a value is not finite, else (lppd mpf, mean longdouble, var longdouble, max |l|,
    max |l - mean|).  Computed once per matrix; the callers share it."""
    out = []
    for k in range(L.shape[1]):
        col = L[:, k]
        if not np.isfinite(col).all():
            out.append(None)
            continue
        v = col.astype(np.longdouble)
        mu = v.sum() / len(v)
        out.append((exact_lppd(col), mu, ((v - mu) ** 2).sum() / len(v), float(np.abs(col).max()), float(np.abs(v - mu).max())))
    return out


def bits_equal(a, b, what=""):
    """bit for bit, except that two NaN are equal whatever their sign and payload (IEEE 754 leaves those of a created NaN to the implementation)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), a[bad][:4], b[bad][:4])


def same_result(a, b, what="", skip=()):
    """two PosteriorWaic with the same bits in every field (skip: data indices left out of the per-datum arrays; the totals then too)"""
    keep = np.ones(len(a.lppd_i), dtype=bool)
    keep[list(skip)] = False
    for f in ("lppd_i", "p_waic_i", "elpd_i", "mean_i", "n_nan", "n_neg_inf", "n_pos_inf"):
        bits_equal(np.asarray(getattr(a, f), dtype=np.float64)[keep], np.asarray(getattr(b, f), dtype=np.float64)[keep], (what, f))
    assert a.n == b.n, what
    if not len(skip):
        for f in ("elpd_waic", "p_waic", "lppd", "se", "waic"):
            bits_equal([getattr(a, f)], [getattr(b, f)], (what, f))
        assert a.n_high_var == b.n_high_var, what


def check_result(res, L, rows_per_part, parts, ranks=1, ref=None, what=""):
    """res: the PosteriorWaic of the matrix L (rows, n_data) = l_is.  The counts and the totals for equality, the columns with a value that
    is not finite against SciPy / NumPy for equality, the finite ones within the module docstring's bounds of the exact reference; prints
    the largest error / bound ratios.  -> the reference (for a second call over the same matrix)"""
    from scipy.special import logsumexp
    L = np.asarray(L, dtype=np.float64)
    n, nd = L.shape
    ref = reference(L) if ref is None else ref
    assert res.n == n and all(getattr(res, f).shape == (nd,) for f in ("lppd_i", "p_waic_i", "elpd_i", "mean_i", "n_nan", "n_neg_inf", "n_pos_inf")), what
    for f, want in (("n_nan", np.isnan(L)), ("n_neg_inf", L == -np.inf), ("n_pos_inf", L == np.inf)):
        assert getattr(res, f).dtype == np.int64 and np.array_equal(getattr(res, f), want.sum(axis=0)), (what, f)
    worst = [0.0, 0.0, 0.0]
    for k in range(nd):
        col = L[:, k]
        if ref[k] is None:
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = (logsumexp(col) - np.log(n), np.var(col), np.mean(col))
            got = (res.lppd_i[k], res.p_waic_i[k], res.mean_i[k])
            if np.isfinite(want[0]):          # some -inf among finite values: the log-sum-exp of the finite ones, within the bound
                fin = col[np.isfinite(col)]
                exact = exact_lppd(fin, n)
                err, bound = abs_error(got[0], exact), lppd_bound(rows_per_part, parts, ranks, float(exact))
                assert err <= bound, (what, k, "lppd_i of a column with -inf", err, bound)
            else:
                assert np.array_equal([got[0]], [want[0]], equal_nan=True), (what, k, "lppd_i", got[0], want[0])
            assert np.array_equal(got[1:], want[1:], equal_nan=True), (what, k, got, want)
            continue
        exact, mu, var, max_abs, D = ref[k]
        err, bound = abs_error(res.lppd_i[k], exact), lppd_bound(rows_per_part, parts, ranks, float(exact))
        bm, bv = trace_bound(n, max_abs, D)
        em, ev = float(abs(np.longdouble(res.mean_i[k]) - mu)), float(abs(np.longdouble(res.p_waic_i[k]) - var))
        worst = [max(worst[0], err / bound), max(worst[1], em / bm), max(worst[2], ev / bv)]
        assert err <= bound, (what, k, "lppd_i", err, bound)
        assert em <= bm, (what, k, "mean_i", em, bm)
        assert ev <= bv, (what, k, "p_waic_i", ev, bv)
    print("%s: rows %d (per part %d, parts %d, ranks %d) x data %d: largest error / bound: lppd_i %.3g, mean_i %.3g, p_waic_i %.3g"
          % (what, n, rows_per_part, parts, ranks, nd, worst[0], worst[1], worst[2]))
    with np.errstate(all="ignore"):
        bits_equal(res.elpd_i, res.lppd_i - res.p_waic_i, (what, "elpd_i"))
        bits_equal([res.elpd_waic, res.p_waic, res.lppd], [np.sum(res.elpd_i), np.sum(res.p_waic_i), np.sum(res.lppd_i)], (what, "totals"))
        bits_equal([res.se, res.waic], [np.sqrt(nd * np.var(res.elpd_i)), -2.0 * np.sum(res.elpd_i)], (what, "se, waic"))
        assert res.n_high_var == int(np.count_nonzero(res.p_waic_i > 0.4)), what
    return ref
