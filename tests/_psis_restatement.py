"""Pareto smoothed importance sampling per column, restated twice from the formulas of the statistic (Vehtari, Simpson, Gelman, Yao and
Gabry; Vehtari, Gelman and Gabry 2017; Zhang and Stephens 2009 with ArviZ's prior): in float64 NumPy, and in mpmath at 200 bits -- the exact
reference of tests/test_psis_host.py and tests/test_gpu_loo.py.  Nothing here knows the library's code.

Per column l (S log densities), x = -l the log ratios:
  M = ceil(min(S / 5, 3 sqrt(S / r_eff))), the kept set the K = min(M + 1, S) smallest l, the cutoff c its largest, x_max = -min(l);
  the tail: the kept values < c, n = tail_len of them; ec = exp(max(-c - x_max, log DBL_MIN));
  n <= 4: k = inf.  Else y = exp(x_tail - x_max) - ec ascending, m = 30 + floor(sqrt(n)), b_j = (1 - sqrt(m / (j - 0.5))) / (3 y_[floor(n / 4
  + 0.5)]) + 1 / y_[n] (1-based), k_j = mean log1p(-b_j y), L_j = n (log(-(b_j / k_j)) - k_j - 1), w_j = 1 / sum_i exp(L_i - L_j), weights below
  10 DBL_EPSILON dropped, the rest normalised, b = sum b_j w_j, k = mean log1p(-b y), sigma = -k / b, k = (n k + 5) / (n + 10);
  k finite: the tail's shifted log ratios become min(0, log(gpinv((j - 0.5) / n, k, sigma) + ec)), j = 1 .. n in rank order;
  elpd = logsumexp(l + lw) - logsumexp(lw): every body draw has l + lw = -x_max, so the numerator is log(n_body exp(-x_max) + sum_tail exp(l +
  lw)) and the denominator needs the body only through logsumexp(-l) over it.

`fit_from_tail` takes what the device's last stage takes -- the sorted kept values and the body's (count, logsumexp(-l)) -- so that stage is
compared on ITS inputs; `column` does a whole column.  Both come in a float64 and an mpmath flavour with the same results dict:
k, sigma, tail_len, smoothed (the tail's log weights, ascending ratio), elpd.

SANITY of the restatement (checked by test_psis_host.py::test_restatement_recovers_the_shape_of_exact_quantiles): on exact generalised Pareto
quantiles, n = 1000, true k in {0.1, 0.5, 0.9}, the estimates are strictly increasing and each lies between the true k and the prior's 0.5
within a margin of 0.002.  Measured here: k_hat = 0.105614, 0.500397, 0.895045 -- 0.1 and 0.9 are pulled towards 0.5 as the prior says (by
0.0056 and 0.0050); at the true k = 0.5 the estimate is 0.0004 above, the profile estimator's own bias on 1000 quantiles, which is what the
margin (five times that) is for."""
import numpy as np

DBL_MIN = np.finfo(np.float64).tiny
EPS = np.finfo(np.float64).eps


def kept(S, r_eff=1.0):
    """K = min(M + 1, S), M = ceil(min(S / 5, 3 sqrt(S / r_eff)))"""
    M = int(np.ceil(min(S / 5.0, 3.0 * np.sqrt(S / float(r_eff)))))
    return min(M + 1, int(S))


def split(col, r_eff=1.0):
    """-> (sorted kept values, body values) of a finite column"""
    col = np.asarray(col, dtype=np.float64)
    K = kept(len(col), r_eff)
    s = np.sort(col)
    c = s[K - 1]
    return s[:K], col[col >= c]


def _gpd_numpy(y, info=None):
    n = len(y)
    m = 30 + int(np.floor(np.sqrt(n)))
    b = 1.0 - np.sqrt(m / (np.arange(1, m + 1) - 0.5))
    b /= 3.0 * y[int(np.floor(n / 4.0 + 0.5)) - 1]
    b += 1.0 / y[-1]
    k = np.log1p(-b[:, None] * y).mean(axis=1)
    L = n * (np.log(-(b / k)) - k - 1.0)
    w = 1.0 / np.exp(L - L[:, None]).sum(axis=1)
    ok = w >= 10.0 * EPS
    if info is not None:
        info["dropped"] = int((~ok).sum())
    w, b = w[ok], b[ok]
    w = w / w.sum()
    bp = np.sum(b * w)
    kp = np.log1p(-bp * y).mean()
    return (n * kp + 5.0) / (n + 10.0), -kp / bp


def fit_from_tail(tail, n_body, body_lse, info=None):
    """float64.  tail: the kept values, ascending; body_lse: logsumexp(-l) over the n_body body draws; info (a dict): takes `dropped`, the
    number of candidate weights under the 10 eps cut"""
    from scipy.special import logsumexp
    with np.errstate(all="ignore"):
        tail = np.asarray(tail, dtype=np.float64)
        l0, c = tail[0], tail[-1]
        t = tail[tail < c]
        n = len(t)
        ec = np.exp(max(l0 - c, np.log(DBL_MIN)))
        xs = (l0 - t)[::-1]                      # the shifted log ratios, ascending
        lt = t[::-1]
        k, sigma, lw = np.inf, np.nan, xs.copy()
        if n > 4:
            k, sigma = _gpd_numpy(np.exp(xs) - ec, info)
            if np.isfinite(k):
                p = np.arange(0.5, n) / n
                if sigma > 0:
                    q = -np.log1p(-p) if abs(k) < EPS else np.expm1(-k * np.log1p(-p)) / k
                    q = q * sigma
                else:
                    q = np.full(n, np.nan)
                lw = np.minimum(np.log(q + ec), 0.0)
        num = logsumexp(np.concatenate([[np.log(float(n_body)) + l0], lt + lw]))
        den = logsumexp(np.concatenate([[body_lse + l0], lw]))
        return dict(k=float(k), sigma=float(sigma), tail_len=n, smoothed=lw, elpd=float(num - den))


def column(col, r_eff=1.0):
    from scipy.special import logsumexp
    tail, body = split(col, r_eff)
    return fit_from_tail(tail, len(body), float(logsumexp(-body)))


def body_lse_exact(body):
    """logsumexp(-l) of the body, mpmath at 200 bits -> mpf"""
    import mpmath as mp
    with mp.workprec(200):
        top = mp.mpf(float(np.max(-np.asarray(body))))
        return top + mp.log(mp.fsum(mp.exp(-mp.mpf(float(v)) - top) for v in body))


def fit_from_tail_exact(tail, n_body, body_lse):
    """mpmath, 200 bits; body_lse: an mpf (body_lse_exact) or a float.  The same decisions (tail, weights dropped, k finite, truncation at 0)
    at that precision.  -> the dict with mpf values (smoothed: a list)"""
    import mpmath as mp
    with mp.workprec(200):
        tl = [mp.mpf(float(v)) for v in tail]
        l0, c = tl[0], tl[-1]
        t = [v for v in tl if v < c]
        n = len(t)
        ec = mp.exp(max(l0 - c, mp.log(mp.mpf(float(DBL_MIN)))))
        lt = t[::-1]
        xs = [l0 - v for v in lt]
        k, sigma, lw = mp.inf, mp.nan, list(xs)
        if n > 4:
            y = [mp.exp(v) - ec for v in xs]
            m = 30 + int(np.floor(np.sqrt(n)))
            yq, yn = y[int(np.floor(n / 4.0 + 0.5)) - 1], y[-1]
            b = [(1 - mp.sqrt(mp.mpf(m) / (mp.mpf(j) - mp.mpf("0.5")))) / (3 * yq) + 1 / yn for j in range(1, m + 1)]
            kj = [mp.fsum(mp.log1p(-bj * v) for v in y) / n for bj in b]
            L = [n * (mp.log(-(bj / kk)) - kk - 1) for bj, kk in zip(b, kj)]
            w = [1 / mp.fsum(mp.exp(Li - Lj) for Li in L) for Lj in L]
            keep = [j for j in range(m) if w[j] >= 10 * mp.mpf(float(EPS))]
            W = mp.fsum(w[j] for j in keep)
            bp = mp.fsum(b[j] * w[j] / W for j in keep)
            kp = mp.fsum(mp.log1p(-bp * v) for v in y) / n
            sigma = -kp / bp
            k = (n * kp + 5) / (n + 10)
            if mp.isfinite(k):
                lw = []
                for j in range(n):
                    p = (mp.mpf(j) + mp.mpf("0.5")) / n
                    if sigma > 0:
                        q = sigma * (-mp.log1p(-p) if abs(k) < mp.mpf(float(EPS)) else mp.expm1(-k * mp.log1p(-p)) / k)
                        lw.append(min(mp.log(q + ec), mp.mpf(0)))
                    else:
                        lw.append(mp.nan)
        num = mp.log(n_body * mp.exp(l0) + mp.fsum(mp.exp(a + b_) for a, b_ in zip(lt, lw)))
        den = mp.log(mp.exp(mp.mpf(body_lse) + l0) + mp.fsum(mp.exp(v) for v in lw))
        return dict(k=k, sigma=sigma, tail_len=n, smoothed=lw, elpd=num - den)


def column_exact(col, r_eff=1.0):
    tail, body = split(col, r_eff)
    return fit_from_tail_exact(tail, len(body), body_lse_exact(body))


def errors(got, exact):
    """(|k - exact|, |sigma - exact| / |exact|, max |smoothed - exact|, |elpd - exact| / max(1, |exact|)) of a float64 result dict against the
    mpmath one, formed at the reference's precision -- elpd_loo_i is a log density of any magnitude (-97 for an outlier), and the rounding of a
    float64 result scales with it; k and the log weights are of order one.  A quantity that is not finite in the reference must be the
    same non-finite value (error 0) or the error is inf"""
    import mpmath as mp

    def one(a, e, rel=None):
        with mp.workprec(200):
            if not mp.isfinite(e):
                same = (mp.isnan(e) and np.isnan(a)) or (mp.isinf(e) and np.isinf(a) and (a > 0) == (e > 0))
                return 0.0 if same else np.inf
            if not np.isfinite(a):
                return np.inf
            d = abs(mp.mpf(float(a)) - e)
            if rel == "rel":
                return float(d / abs(e))
            if rel == "rel1":
                return float(d / max(mp.mpf(1), abs(e)))
            return float(d)
    assert got["tail_len"] == exact["tail_len"], (got["tail_len"], exact["tail_len"])
    sm = max([one(a, e) for a, e in zip(got["smoothed"], exact["smoothed"])] or [0.0])
    return one(got["k"], exact["k"]), one(got["sigma"], exact["sigma"], rel="rel"), sm, one(got["elpd"], exact["elpd"], rel="rel1")


QUANTITIES = ("k", "sigma (relative)", "smoothed tail", "elpd (relative to max(1, |elpd|))")


def recorded_bound(path=None):
    """profiles/psis_bound.txt (tools/psis_bound.py) -> {quantity: (the NumPy restatement's largest error, the gate = 4 x it)}"""
    import os
    import re
    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "psis_bound.txt")
    out = {}
    for line in open(path):
        m = re.match(r"^(.+?)\s+(\S+e[-+]\d+) \(.*?\) \| (\S+e[-+]\d+) \(.*?\) \| (\S+e[-+]\d+)$", line.rstrip())
        if m and not line.startswith("#"):
            out[m.group(1)] = (float(m.group(2)), float(m.group(4)))
    assert sorted(out) == sorted(QUANTITIES), (path, sorted(out))
    return out


def gpd_quantiles(n, k, sigma=1.0):
    """exact quantiles of the generalised Pareto distribution at (j - 0.5) / n, ascending"""
    p = np.arange(0.5, n) / n
    return sigma * np.expm1(-k * np.log1p(-p)) / k


def tail_from_excesses(z, l0=-5.0, ec=0.01):
    """kept values (ascending) whose PSIS inputs y = exp(l0 - l) - exp(l0 - c) are the positive excesses z up to a common scale (the fit's k
    does not depend on it): the shifted ratios are r = z (1 - ec) / max(z) + ec in (ec, 1], l = l0 - log(r), and the cutoff c = l0 - log(ec)
    is the largest kept value"""
    z = np.asarray(z, dtype=np.float64)
    r = z * ((1.0 - ec) / z.max()) + ec
    return np.concatenate([np.sort(l0 - np.log(r)), [l0 - np.log(ec)]])


def host_cases():
    """[(name, kept values ascending, n_body, m_b, s_b)]: the cases of tests/test_psis_host.py and tools/psis_bound.py.  Tails of n = 5, 6, 29, 30,
    31, 255, 256, 257 draws of a generalised Pareto distribution (k = 0.5, seeded); a tail of equal values except one; exponential
    quantiles (k near 0) and quantiles of k = 1.2; 4000 quantiles of k = 0.3, where most candidate weights fall under the 10 eps cut; and
    tails of 4 and 0 values, which are not smoothed; and the columns the GPU tests themselves fit at their two shortest fitted windows
    (tests/test_gpu_loo.py: the last 21 and 224 rows of make_history(130, 16, 3) under source 3 and make_data(5, 3): tails of 5 and 45
    log densities of a posterior-like cloud).  The fit of a tail of 5 such values is the worst conditioned thing the tests meet -- the float64
    restatement's own k is off by 3.5e-14 there, four times its error on any synthetic tail above -- and a gate that is to say something
    about those columns has to be measured on them.  The body: n_body draws at the cutoff and below the tail's ratios (the columns: their own
    body), (m_b, s_b) as the device's second pass would hand them over, in float64."""
    rs = np.random.RandomState(2024)
    out = []

    def add(name, tail, n_body=None, body=None):
        n_body = (4 * len(tail) if n_body is None else n_body) if body is None else len(body)
        if body is None:
            body = np.concatenate([[tail[-1]], tail[-1] + rs.exponential(2.0, size=n_body - 1)])
        m_b = float(np.max(-body))
        out.append((name, tail, n_body, m_b, float(np.sum(np.exp(-body - m_b)))))
    for n in (5, 6, 29, 30, 31, 255, 256, 257):
        u = rs.uniform(size=n)
        add("gpd draws n=%d" % n, tail_from_excesses(np.expm1(-0.5 * np.log1p(-u)) / 0.5))
    add("equal but one", tail_from_excesses(np.array([1.0] * 39 + [3.0])))
    add("exponential", tail_from_excesses(-np.log1p(-np.arange(0.5, 100) / 100)))
    add("k=1.2", tail_from_excesses(gpd_quantiles(100, 1.2)))
    add("weights cut", tail_from_excesses(gpd_quantiles(4000, 0.3)), n_body=16000)
    add("tail of 4", tail_from_excesses(np.array([1.0, 2.0, 3.0, 4.0])))
    add("tail of 0", np.array([-2.0]), n_body=7)
    import _waic_cases as WC
    X = WC.make_history(130, 16, 3).reshape(-1, 3)
    pw = WC.pointwise(3, WC.make_data(5, 3))
    for rows in (21, 224):
        L = pw(X[len(X) - rows:])
        for i in range(L.shape[1]):
            tail, body = split(L[:, i])
            add("window of %d rows, datum %d" % (rows, i), tail, body=body)
    return out


def case_exact(case):
    """the mpmath result of one of host_cases(), the body's log-sum-exp formed from the float64 (m_b, s_b) the code under test is given"""
    import mpmath as mp
    _, tail, n_body, m_b, s_b = case
    with mp.workprec(200):
        lse = mp.mpf(m_b) + mp.log(mp.mpf(s_b))
    return fit_from_tail_exact(tail, n_body, lse)
