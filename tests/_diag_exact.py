"""An exact statement of what bpm_diag_split_moments / bpm_diag_autocov return for one rank's block H[rows, n_local, d] over the window
[g0, g1), and the bound on what the device's float64 evaluation (bipymc_amd/csrc/diagnostics.h) may differ from it by.  A plain module: no
GPU, no library; tests/test_diag_exact_host.py tests it, tests/test_gpu_diagnostics_edges.py holds the kernels to it.

WHAT IS COMPUTED (the definitions of bipymc_amd/diagnostics.py).  n = (g1 - g0) // 2; half 0 = rows [g0, g0 + n), half 1 = rows [g1 - n, g1);
m = 2 n_local half-chains j with values x_{j,0..n-1}, mean xbar_j, centred values y_{j,i} = x_{j,i} - xbar_j.  Per coordinate
    mean   = (1/m) sum_j xbar_j                               m2 = sum_j (xbar_j - mean)^2
    sum_var = sum_j (1/(n-1)) sum_i y_{j,i}^2                 c[t] = sum_j (1/n) sum_{i=0}^{n-1-t} y_{j,i} y_{j,i+t},  t = 0 ... n - 1

HOW.  Every double of a column is an integer times one power of two 2^e (e = the column's smallest exponent), so with X the integers,
S_j = sum_i X_{j,i}, T = sum_j S_j and Y_{j,i} = n X_{j,i} - S_j, each quantity is one integer over an integer times 2^e or 2^2e:
    mean = T / (n m);  m2 = sum_j (m S_j - T)^2 / (n m)^2;  sum_var = sum_j (n sum_i X^2 - S_j^2) / (n (n-1));  c[t] = sum_j sum_i Y_{j,i} Y_{j,i+t} / n^3.
The integers are Python's (unbounded), the quotient a fractions.Fraction, and float(Fraction) rounds once, correctly: every returned double is
the exactly rounded value of the definition -- what math.fsum over Fraction products would give, without forming the Fractions one by one.
np.longdouble is not used anywhere (where its eps is 2^-52 it would be no reference at all, and a 64-bit significand does not hold a product
of two doubles either).

NON-FINITE VALUES.  A coordinate with a NaN or +-inf in either half has NaN in all of its outputs; every other coordinate is computed from
its own column alone and is what it would be without that value.  Rows outside the two halves (the middle row of an odd window, rows before
g0) are not read.

THE BOUND.  u = 2^-53, eta = 2^-1074 (the spacing of the subnormals: every multiplication, division or fma whose result is subnormal errs by at
most eta / 2 more; additions and subtractions never underflow inexactly), gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1: a sum of k + 1 terms added in ANY order errs by at most gamma_k sum |terms|; the kernels' orders are
fixed, but the bound does not depend on which).  The library is built without contraction, so a product is rounded unless written as fma.

 (a) a half-chain's mean (diag_split_moments_kernel).  s = x_0 is the shift, d_i = x_i - s exactly, A = sum_i |d_i|, Q = sum_i d_i^2.
     The kernel rounds d_i (u |d_i|), adds the n of them in sequence (gamma_{n-1} sum |d^_i|), multiplies by the rounded 1/n (2 u, eta) and
     adds s (u |result|):
         |xbar^_j - xbar_j| <= delta_j := gamma_{n+3} A_j / n + 2 eta + u |xbar_j|          (A / n <= max |x - x_first|)
 (b) a half-chain's M2 = sb - sa * m0, clamped at 0 (the exact value is >= 0, so the clamp moves towards it).  sb = sum fl(d^_i^2):
     |sb - Q| <= gamma_{n+2} Q + n eta.  sa = sum d + e1, |e1| <= gamma_n A;  m0 = sum d / n + e2, |e2| <= gamma_{n+2} A / n + eta;  with
     |sum d| <= A the product differs from (sum d)^2 / n by at most gamma_{2n+5} A^2 / n + (A + 1) eta, its rounding included.  The last
     subtraction adds u |M2^|:
         |M2^_j - M2_j| <= E_j := (1 + u) (gamma_{n+2} Q_j + gamma_{2n+5} A_j^2 / n + (n + A_j + 1) eta) + u M2_j
     The shift makes this independent of the column's offset: Q and A^2 / n are of the size of M2 itself unless the half's first value is far
     from the rest of it.
 (c) diag_means_final_kernel: m terms in a fixed order, M2 / (n - 1) rounded before it is added, the mean divided by m:
         |sum_var^ - sum_var| <= (sum_j E_j + gamma_m sum_j (M2_j + E_j)) / (n - 1) + m eta
         |mean^ - mean|       <= delta_mu := (1/m) sum_j delta_j + gamma_m (1/m) sum_j (|xbar_j| + delta_j) + eta
     e^_j = fl(xbar^_j - mean^) differs from e_j = xbar_j - mean by at most eps_j := (1 + u) (delta_j + delta_mu) + u |e_j|, and
     sum (e + eps)^2 - sum e^2 <= sum (2 |e| eps + eps^2); the m rounded squares are then added:
         |m2^ - m2| <= sum_j (2 |e_j| eps_j + eps_j^2) + gamma_{m+1} sum_j (|e_j| + eps_j)^2 + m eta
 (d) diag_autocov_kernel centres on the ROUNDED mean xbar^_j = xbar_j + D, |D| <= delta_j.  In exact arithmetic
         sum_{i=0}^{n-1-t} (y_i - D)(y_{i+t} - D) - sum y_i y_{i+t} = -D (sum_{i<n-t} y_i + sum_{i>=t} y_i) + (n - t) D^2,
     and because sum_{i<n} y_i = 0 each of the two sums is minus a sum of t of the y: at most t Ymax_j.  So the lag-t sum of half-chain j
     moves by at most 2 t delta_j Ymax_j + (n - t) delta_j^2 -- by n delta^2 alone at t = 0 -- before the division by n.  The kernel then
     rounds each y^ (u each), accumulates the T = m (n - t) products with one rounding per fma, adds lanes, workgroups and slices in a fixed
     order and divides by n: gamma_{T+3}; one more (gamma_{T+4}) so that the bound also holds for an evaluation that rounds the products, as
     the float64 model of tests/test_diag_exact_host.py does.  Zeros (idle lanes, the ring before the half's first row) add exactly.
         |c^[t] - c[t]| <= (1/n) sum_j (2 t delta_j Ymax_j + (n - t) delta_j^2)
                           + gamma_{T+4} (1/n) sum_j sum_i (|y_{j,i}| + delta_j)(|y_{j,i+t}| + delta_j) + (T + 1) eta
     At offset 1e8 and unit spread delta ~ 1e8 u = 1.1e-8: c[t >= 1] is good to ~ 2 t delta / n per half-chain, c[0] to delta^2 ~ 1e-16.

The bound itself is evaluated in float64 from the data (its terms are sums of non-negative numbers: relative error ~ n u, and Ymax_j is taken
as max |x - fl(xbar_j)| + delta_j) and multiplied by 1 + 2^-20 to stay an upper bound.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
ETA = 2.0 ** -1074
KEYS = ("mean", "m2", "sum_var", "c")


def gamma(k):
    return k * U / (1.0 - k * U)


def halves(H, g0, g1):
    """-> (n, 2 n_local, d): the half-chains of the window side by side, j = half * n_local + chain"""
    H = np.asarray(H, dtype=np.float64)
    n = (int(g1) - int(g0)) // 2
    if n < 4:
        raise ValueError("a window of %d rows gives half-chains of %d draws; at least 4 are needed" % (g1 - g0, n))
    return np.concatenate([H[g0:g0 + n], H[g1 - n:g1]], axis=1)


def _to_ints(h):
    """h (n, m, d) finite -> (X, e): Python integers X (an object array) and per column e with h[:, :, k] == X[:, :, k] * 2^e[k] exactly"""
    mant, ex = np.frexp(h)
    M = np.ldexp(mant, 53).astype(np.int64)          # |mant| in [1/2, 1): an integer below 2^53, exactly
    ex = ex.astype(np.int64) - 53
    nz = h != 0
    big = np.iinfo(np.int64).max
    e = np.where(nz, ex, big).min(axis=(0, 1))
    e = np.where(e == big, 0, e)
    sh = np.where(nz, ex - e, 0)
    X = np.empty(h.size, dtype=object)
    X[:] = [a << b for a, b in zip(M.ravel().tolist(), sh.ravel().tolist())]
    return X.reshape(h.shape), [int(v) for v in e]


def _floats(num, den, e, power):
    """num: (d,) integers -> float(num / den * 2^(power e)), rounded once"""
    return np.array([float(Fraction(int(a), den) * Fraction(2) ** (power * ek)) for a, ek in zip(num, e)], dtype=np.float64)


def exact(H, g0, g1):
    """-> dict(mean, m2, sum_var: (d,); c: (n, d), every lag 0 ... n - 1; n, m)"""
    h = halves(H, g0, g1)
    n, m, d = h.shape
    bad = ~np.isfinite(h).all(axis=(0, 1))
    X, e = _to_ints(np.where(bad, 0.0, h))
    S = X.sum(axis=0)                                # (m, d)
    T = S.sum(axis=0)
    dev = m * S - T
    Y = n * X - S
    out = dict(n=n, m=m,
               mean=_floats(T, n * m, e, 1),
               m2=_floats((dev * dev).sum(axis=0), (n * m) ** 2, e, 2),
               sum_var=_floats((n * (X * X).sum(axis=0) - S * S).sum(axis=0), n * (n - 1), e, 2),
               c=np.stack([_floats((Y[:n - t] * Y[t:]).sum(axis=0).sum(axis=0), n ** 3, e, 2) for t in range(n)]))
    for key in KEYS:
        out[key][..., bad] = np.nan
    return out


def bound(H, g0, g1):
    """-> dict(mean, m2, sum_var: (d,); c: (n, d)): the most the device's values may differ from exact()'s (NaN for a non-finite coordinate)"""
    h = halves(H, g0, g1)
    n, m, d = h.shape
    with np.errstate(invalid="ignore", over="ignore"):
        dd = h - h[0]
        A = np.abs(dd).sum(axis=0)                   # (m, d)
        Q = (dd * dd).sum(axis=0)
        xbar = h[0] + dd.sum(axis=0) / n
        delta = gamma(n + 3) * A / n + 2 * ETA + U * np.abs(xbar)
        M2 = np.maximum(Q - dd.sum(axis=0) ** 2 / n, 0.0)
        E = (1 + U) * (gamma(n + 2) * Q + gamma(2 * n + 5) * A * A / n + (n + A + 1) * ETA) + U * M2
        sum_var = (E.sum(axis=0) + gamma(m) * (M2 + E).sum(axis=0)) / (n - 1) + m * ETA
        delta_mu = delta.sum(axis=0) / m + gamma(m) * (np.abs(xbar) + delta).sum(axis=0) / m + ETA
        e = np.abs(xbar - xbar.sum(axis=0) / m) + delta + delta_mu       # |e_j|, from above
        eps = (1 + U) * (delta + delta_mu) + U * e
        m2 = (2 * e * eps + eps * eps).sum(axis=0) + gamma(m + 1) * ((e + eps) ** 2).sum(axis=0) + m * ETA
        y = np.abs(h - xbar) + delta                 # (n, m, d): |y_{j,i}| + delta_j, from above
        ymax = y.max(axis=0)
        c = np.empty((n, d))
        for t in range(n):
            T = m * (n - t)
            c[t] = ((2 * t * delta * ymax + (n - t) * delta * delta).sum(axis=0) + gamma(T + 4) * (y[:n - t] * y[t:]).sum(axis=(0, 1))) / n \
                + (T + 1) * ETA
    out = dict(mean=delta_mu, m2=m2, sum_var=sum_var, c=c)
    bad = ~np.isfinite(h).all(axis=(0, 1))
    for key in KEYS:
        out[key] = out[key] * (1.0 + 2.0 ** -20)
        out[key][..., bad] = np.nan
    return out


def worst_ratios(got, ref, bnd):
    """got, ref, bnd: dicts over KEYS (c of equal shapes).  NaN must sit where the reference has it; -> {key: largest |got - ref| / bound}"""
    worst = {}
    for key in KEYS:
        g, r, b = np.asarray(got[key]), np.asarray(ref[key]), np.asarray(bnd[key])
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(g), nan), (key, np.argwhere(np.isnan(g) != nan)[:4])
        assert np.all(b[~nan] > 0)
        worst[key] = float(np.max(np.abs(g - r)[~nan] / b[~nan])) if (~nan).any() else 0.0
    return worst
