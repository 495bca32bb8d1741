"""The test likelihood of the per-datum form of HipLikelihood (bipymc_amd/csrc/user_eval_data.h), its exact value and the bound on what the
device's float64 evaluation may differ from it by.  A plain module: no GPU, no library; tests/test_data_likelihood_host.py tests it,
tests/test_gpu_data_likelihood.py holds the kernels to it.

THE LIKELIHOOD.  A polynomial fit: datum i has an abscissa t_i and a value y_i (w = 1: the data carry only y and t_i = i; w = 3: the columns
are t, y and one more that the model does not read), the row x has d >= 3 coordinates, p = [p0, p1]:
    r_i = y_i - (x0 + x1 t_i + x2 (t_i t_i))          acc[0] += (r_i r_i) p0          K >= 2:  acc[1] += r_i
    total = -0.5 acc[0]  (+ p1 acc[1], K >= 2)  - 0.5 (x[d-1] x[d-1])            (the last term: a mis-staged wide row shows)
and with K > 2 ln_like_total returns NaN unless acc[2 .. K) are still exactly zero.  hip_source(K, w) is the HIP statement, python_fn(...) the
NumPy one (the contract of HipLikelihood's python_fn: the same function for the host and for the CPU test engine).

THE EXACT VALUE.  sum r^2 and sum r are polynomials in x whose coefficients are the nine data moments sum 1, t, t^2, t^3, t^4, y, y t, y t^2, y^2:
    sum r   = Sy - n x0 - x1 St - x2 St2
    sum r^2 = Sy2 - 2 x0 Sy - 2 x1 Syt - 2 x2 Syt2 + n x0^2 + 2 x0 x1 St + (2 x0 x2 + x1^2) St2 + 2 x1 x2 St3 + x2^2 St4
Moments accumulates them as fractions.Fraction of the float inputs (every double is a rational), exact_value() evaluates the polynomials and the
total in Fractions of the float x and p, and float(Fraction) rounds once, correctly.  np.longdouble is used nowhere.  exact_value_termwise() is the
definition itself, datum by datum in Fractions: the host test holds the moment form to it.

THE BOUND.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a value that went through
k roundings carries a factor (1 + theta), |theta| <= gamma_k; a sum in which every term passes through at most k additions, in ANY order, errs by at
most gamma_k sum |terms|).  A fused multiply-add rounds once where the unfused pair rounds twice, so a count of the unfused roundings is an upper
count for every contraction the compiler may choose: the bound holds with and without -ffp-contract.
 (a) r_i.  The operands reach r through at most 5 roundings (x2: t t, x2 *, +, -  = 4;  x1: *, +, +, - = 4;  x0: +, +, - = 3;  y: - = 1; one spare):
         |r^_i - r_i| <= D_i := gamma_5 A_i,     A_i = |y_i| + |x0| + |x1 t_i| + |x2 t_i^2|
     (an absolute bound through the magnitudes: where the model cancels the data, r is small and its RELATIVE error is not).
 (b) the term T_i = r_i^2 p0: two more roundings.  With R_i := |r^_i| + D_i >= max(|r_i|, |r^_i|):
         |T^_i - T_i| <= e_i := |p0| ((2 R_i D_i + D_i^2) (1 + gamma_2) + gamma_2 R_i^2),      |T^_i| <= M_i := |p0| R_i^2 (1 + gamma_2)
 (c) the sum.  A term is added at most ceil(C / 64) times in its lane (C = the chunk, bpm_data_likelihood_chunk()), 6 times in the butterfly and
     n_chunks = ceil(n_data / C) times in the fold of the chunk sums: depth = ceil(C / 64) + 6 + n_chunks (with one chunk there is no fold and the
     first addition of a lane, to 0.0, is exact: counted all the same).
         |acc^[0] - sum T_i| <= E0 := (1 + gamma_depth) sum e_i + gamma_depth sum M_i
         |acc^[1] - sum r_i| <= E1 := (1 + gamma_depth) sum D_i + gamma_depth sum R_i
 (d) the total: -0.5 acc[0] is exact, p1 acc[1] one rounding, x_l^2 one, 0.5 x_l^2 exact, and at most two additions on any operand's way (3 roundings):
         |total^ - total| <= (0.5 E0 + |p1| E1) (1 + gamma_3) + gamma_3 (0.5 sum M_i + |p1| sum R_i + 0.5 x_l^2)
 (e) underflow: a product whose result is subnormal errs by at most eta / 2 = 2^-1075 more; a term has 6 products: + 6 n eta, far below everything
     else for the inputs used here, kept so that the bound is a bound.
error_bound() evaluates (a) - (e) in float64 NumPy from the float inputs; that evaluation itself errs by a relative 1e-12 or so, and the result is
multiplied by 1.001.
python_fn obeys the same bound: its terms are the same expressions, and NumPy's sum (blocks of at most 128 elements in 8 interleaved accumulators,
the blocks pairwise: at most 16 + 3 + log2(n / 128) additions on a term's way, 27 at n = 2^15) is shallower than `depth` >= 71.  So a device value
and a python_fn value of the same row differ by at most twice the bound.  No tolerance here is tuned on a GPU."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
ETA = 2.0 ** -1074


def gamma(k):
    return k * U / (1.0 - k * U)


def hip_source(K, w):
    """the per-datum source (what HipLikelihood(..., data=, terms=K) takes: it prepends BPM_LN_LIKE_DATA / BPM_LN_LIKE_DATA_W itself)"""
    t, y = ("(double)i", "y[0]") if w == 1 else ("y[0]", "y[1]")
    return ("__device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc) {\n"
            "    const double t = %s;\n"
            "    const double r = %s - (x[0] + x[1] * t + x[2] * (t * t));\n"
            "    acc[0] += r * r * p[0];\n%s}\n"
            "__device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p) {\n"
            "    for (int k = 2; k < BPM_LN_LIKE_DATA; ++k) if (acc[k] != 0.0) return NAN;\n"
            "    double v = -0.5 * acc[0];\n%s"
            "    return v - 0.5 * (x[d - 1] * x[d - 1]);\n}\n") % (t, y, "    acc[1] += r;\n" if K >= 2 else "", "    v += p[1] * acc[1];\n" if K >= 2 else "")


def plain_source(K, n_data):
    """the same likelihood in the PLAIN form, its data inside params: p = [p0, p1, t_0, y_0, t_1, y_1, ...]; one lane walks the data in order"""
    return ("__device__ double ln_like(const double* x, int d, const double* p) {\n"
            "    double a0 = 0.0, a1 = 0.0;\n"
            "    for (int i = 0; i < %d; ++i) {\n"
            "        const double t = p[2 + 2 * i];\n"
            "        const double r = p[3 + 2 * i] - (x[0] + x[1] * t + x[2] * (t * t));\n"
            "        a0 += r * r * p[0]; a1 += r;\n    }\n"
            "    double v = -0.5 * a0;\n%s"
            "    return v - 0.5 * (x[d - 1] * x[d - 1]);\n}\n") % (n_data, "    v += p[1] * a1;\n" if K >= 2 else "")


def split(data):
    """data (n_data,) or (n_data, w) -> (t, y) float64"""
    data = np.asarray(data, dtype=np.float64)
    if data.ndim == 1 or data.shape[1] == 1:
        y = data.reshape(-1)
        return np.arange(len(y), dtype=np.float64), y.copy()
    return data[:, 0].copy(), data[:, 1].copy()


def python_fn(K, data, p):
    """theta -> float: the NumPy statement of the same formula"""
    t, y = split(data)
    p = np.asarray(p, dtype=np.float64)

    def fn(theta):
        x = np.asarray(theta, dtype=np.float64).reshape(-1)
        r = y - (x[0] + x[1] * t + x[2] * (t * t))
        v = -0.5 * np.sum(r * r * p[0])
        if K >= 2:
            v += p[1] * np.sum(r)
        return float(v - 0.5 * (x[-1] * x[-1]))
    return fn


def make_data(n_max, w, seed=11):
    """the data of every case with this w: the cases with fewer data points take the first n_data rows.  w = 1: y around a parabola in t = i;
    w = 3: t uniform in [0, 1), y around a parabola in t, a third column the model does not read."""
    rs = np.random.RandomState(seed + w)
    if w == 1:
        i = np.arange(n_max, dtype=np.float64)
        return 1.5 - 2e-3 * i + 3e-7 * i * i + 0.3 * rs.normal(size=n_max)
    t = rs.uniform(size=n_max)
    return np.column_stack([t, 0.5 + 2.0 * t - 1.5 * t * t + 0.3 * rs.normal(size=n_max), rs.normal(size=n_max)])


def x_scale(w):
    """the size of x0, x1, x2 at which the model is of the size of the data"""
    return np.array([1.0, 1e-3, 1e-7]) if w == 1 else np.array([1.0, 1.0, 1.0])


def make_rows(n, d, w, seed=5):
    """n rows of d coordinates: the model's three coordinates near the data's parabola, the others of order one"""
    rs = np.random.RandomState(seed + 7 * d)
    X = rs.normal(size=(n, d))
    centre = np.array([1.5, -2.0, 3.0]) if w == 1 else np.array([0.5, 2.0, -1.5])
    X[:, :3] = (centre + 0.2 * rs.normal(size=(n, 3))) * x_scale(w)
    return X


class Moments(object):
    """the nine exact data moments at the prefixes `sizes` of the data: at[n] = (S1, St, St2, St3, St4, Sy, Syt, Syt2, Sy2) over the first n data"""

    def __init__(self, data, sizes):
        t, y = split(data)
        want = set(int(n) for n in sizes)
        assert max(want) <= len(y) and min(want) >= 1
        acc = [Fraction(0)] * 9
        self.at = {}
        for i in range(max(want)):
            ti, yi = Fraction(float(t[i])), Fraction(float(y[i]))
            t2 = ti * ti
            terms = (1, ti, t2, t2 * ti, t2 * t2, yi, yi * ti, yi * t2, yi * yi)
            acc = [a + b for a, b in zip(acc, terms)]
            if i + 1 in want:
                self.at[i + 1] = tuple(acc)


def exact_sums(x, mom):
    """-> (sum r^2, sum r) as Fractions from the moments `mom` of one prefix"""
    x0, x1, x2 = (Fraction(float(v)) for v in x[:3])
    n, St, St2, St3, St4, Sy, Syt, Syt2, Sy2 = mom
    s1 = Sy - n * x0 - x1 * St - x2 * St2
    s2 = (Sy2 - 2 * x0 * Sy - 2 * x1 * Syt - 2 * x2 * Syt2 + n * x0 * x0 + 2 * x0 * x1 * St + (2 * x0 * x2 + x1 * x1) * St2 + 2 * x1 * x2 * St3 +
          x2 * x2 * St4)
    return s2, s1


def exact_value(x, mom, p, K):
    """the correctly rounded total of row x over the prefix whose moments are `mom`"""
    s2, s1 = exact_sums(x, mom)
    xl = Fraction(float(x[-1]))
    v = -Fraction(1, 2) * s2 * Fraction(float(p[0])) - Fraction(1, 2) * xl * xl
    if K >= 2:
        v += Fraction(float(p[1])) * s1
    return float(v)


def exact_value_termwise(x, data, p, K):
    """the definition, datum by datum in Fractions (slow: small n only)"""
    t, y = split(data)
    x0, x1, x2 = (Fraction(float(v)) for v in x[:3])
    s2 = s1 = Fraction(0)
    for ti, yi in zip(t, y):
        ti = Fraction(float(ti))
        r = Fraction(float(yi)) - (x0 + x1 * ti + x2 * ti * ti)
        s2 += r * r
        s1 += r
    xl = Fraction(float(x[-1]))
    v = -Fraction(1, 2) * s2 * Fraction(float(p[0])) - Fraction(1, 2) * xl * xl
    if K >= 2:
        v += Fraction(float(p[1])) * s1
    return float(v)


def depth(n_data, chunk):
    return -(-chunk // 64) + 6 + -(-n_data // chunk)


def error_bound(x, data, p, K, chunk):
    """the docstring's bound (a) - (e) for row x over `data` (all of it), the device's chunk being `chunk`"""
    t, y = split(data)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = len(y)
    g2, g3, g5, gd = gamma(2), gamma(3), gamma(5), gamma(depth(n, chunk))
    A = np.abs(y) + abs(x[0]) + np.abs(x[1] * t) + np.abs(x[2] * (t * t))
    D = g5 * A
    R = np.abs(y - (x[0] + x[1] * t + x[2] * (t * t))) + D
    p0, p1 = abs(float(p[0])), (abs(float(p[1])) if K >= 2 else 0.0)
    e = p0 * ((2.0 * R * D + D * D) * (1.0 + g2) + g2 * R * R)
    M = p0 * R * R * (1.0 + g2)
    sM, sR = math.fsum(M), math.fsum(R)
    E0 = (1.0 + gd) * math.fsum(e) + gd * sM
    E1 = (1.0 + gd) * math.fsum(D) + gd * sR
    xl2 = float(x[-1]) ** 2
    b = (0.5 * E0 + p1 * E1) * (1.0 + g3) + g3 * (0.5 * sM + p1 * sR + 0.5 * xl2) + 6.0 * n * ETA
    return 1.001 * b
