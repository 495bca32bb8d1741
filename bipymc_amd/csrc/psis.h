// PARETO SMOOTHED IMPORTANCE SAMPLING PER DATUM, fit and finish: from the sorted tail of a datum's log densities (pointwise_tail.h, stage A) and the
// log-sum-exp of the rest (stage B) to pareto_k, sigma, the smoothed tail, tail_len and elpd_loo_i (Vehtari, Simpson, Gelman, Yao and Gabry,
// "Pareto smoothed importance sampling"; Vehtari, Gelman and Gabry 2017; Zhang and Stephens 2009 for the fit).  bipymc_amd/pointwise.py:
// param_est_loo states what comes out.  Everything but the __global__ wrappers at the end is plain C++ (tests/psis_host_main.cpp runs it on the host).
//
// A datum is worked on by a TEAM of PSIS_THREADS = 256 lanes (a workgroup on the device; a loop on the host), and THE ORDER OF EVERY SUM IS FIXED:
//   psis_sum(n, f):  lane t adds f(t), f(t + 256), f(t + 512), ... in that order to 0; then red[t] += red[t + off] for off = 128, 64, ..., 1.
//   Sums over the m <= 30 + sqrt(n) candidates of the fit run over j = 0, 1, 2, ... serially, the same in every lane.
// The steps, with l_0 <= l_1 <= ... the kept values (n_kept of them, ascending), c = l_[n_kept - 1] the cutoff, x_max = -l_0:
//   1. n = tail_len = how many kept values are < c (ties with the cutoff belong to the body).  ec = exp(max(l_0 - c, log DBL_MIN)).
//   2. n <= 4: k = +inf, nothing is smoothed.  Else y_j = exp(l_0 - l_[n - 1 - j]) - ec, j = 0 .. n - 1 (ascending), and with m = 30 + floor(sqrt(n)):
//        b_j = (1 - sqrt(m / (j + 0.5))) / (3 y_[floor(n / 4 + 0.5) - 1]) + 1 / y_[n - 1];   k_j = psis_sum_i log1p(-b_j y_i) / n;
//        L_j = n (log(-(b_j / k_j)) - k_j - 1);   w_j = 1 / sum_i exp(L_i - L_j);   w_j < 10 DBL_EPSILON dropped;   W = sum_j w_j;
//        b = sum_j b_j (w_j / W);   k = psis_sum_i log1p(-b y_i) / n;   sigma = -k / b;   k = (n k + 5) / (n + 10).
//   3. k finite: lw_j = min(0, log(gpinv((j + 0.5) / n, k, sigma) + ec)) replaces the shifted log ratio l_0 - l_[n - 1 - j] of the tail's j-th smallest
//      ratio; gpinv(p, k, sigma) = sigma expm1(-k log1p(-p)) / k (|k| < DBL_EPSILON: -sigma log1p(-p)), NaN for sigma <= 0.
//   4. With t_j = l_[n - 1 - j] + lw_j, (n_b, m_b, s_b) the body's count and log-sum-exp of -l (m_b + log s_b), A = max(l_0, max_j t_j), B = max(m_b + l_0, max_j lw_j):
//        elpd = (A + log(n_b exp(l_0 - A) + psis_sum_j exp(t_j - A))) - (B + log(s_b exp((m_b + l_0) - B) + psis_sum_j exp(lw_j - B))).
//      (Every body draw has l + lw = -x_max = l_0 exactly, so the numerator's body term is n_b exp(l_0).)
// Work space per datum: n doubles (y, then lw) and 3 m doubles (b, L, w).
#pragma once
#include "pointwise_rows.h"      // BPM_PW_HD, pw_merge_lse

#include <float.h>
#include <math.h>
#include <stdint.h>

namespace bpm {
inline namespace BPM_VARIANT_NS {

constexpr uint32_t PSIS_THREADS = 256;
constexpr double PSIS_BAD_K = 0.7;

// fields of bpm_loo's records: counts are 64-bit words, the rest doubles
enum { LOO_ELPD = 0, LOO_K, LOO_SIGMA, LOO_TAIL_LEN, LOO_KEPT, LOO_BODY_N, LOO_BODY_M, LOO_BODY_S, LOO_FIELDS };

// M = ceil(min(S / 5, 3 sqrt(S / r_eff))) draws are smoothed at most; the kept set is the K = min(M + 1, S) smallest.  -> K (0 for S = 0)
inline uint64_t psis_kept(uint64_t S, double r_eff) {
    if (S == 0) return 0;
    const double a = (double)S / 5.0, b = 3.0 * sqrt((double)S / r_eff);
    const double M = ceil(a < b ? a : b);
    return M + 1.0 < (double)S ? (uint64_t)M + 1 : S;
}
inline uint32_t psis_candidates(uint64_t n) { return 30u + (uint32_t)floor(sqrt((double)n)); }
// doubles of work space for a datum whose kept set has K values
inline uint64_t psis_work(uint64_t K) { return K + 3ull * psis_candidates(K); }

struct PsisTeam { double* red; };      // PSIS_THREADS doubles: LDS on the device

BPM_PW_HD bool psis_lane0() {
#if defined(__HIP_DEVICE_COMPILE__)
    return threadIdx.x == 0;
#else
    return true;
#endif
}
BPM_PW_HD void psis_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

template <class F>
BPM_PW_HD double psis_sum(const PsisTeam& tm, uint32_t n, F f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = threadIdx.x;
    double a = 0.0;
    for (uint32_t i = t; i < n; i += PSIS_THREADS) a += f(i);
    __syncthreads();      // (the previous result has been read by every lane)
    tm.red[t] = a;
    __syncthreads();
    for (uint32_t off = PSIS_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) tm.red[t] += tm.red[t + off];
        __syncthreads();
    }
    return tm.red[0];
#else
    for (uint32_t t = 0; t < PSIS_THREADS; ++t) {
        double a = 0.0;
        for (uint32_t i = t; i < n; i += PSIS_THREADS) a += f(i);
        tm.red[t] = a;
    }
    for (uint32_t off = PSIS_THREADS / 2; off > 0; off >>= 1)
        for (uint32_t t = 0; t < off; ++t) tm.red[t] += tm.red[t + off];
    return tm.red[0];
#endif
}

// the largest f(i), i < n, and `floor` (no f is NaN where this is called with one that matters: a NaN loses every comparison)
template <class F>
BPM_PW_HD double psis_max(const PsisTeam& tm, uint32_t n, double floor_, F f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = threadIdx.x;
    double a = floor_;
    for (uint32_t i = t; i < n; i += PSIS_THREADS) { const double v = f(i); a = v > a ? v : a; }
    __syncthreads();
    tm.red[t] = a;
    __syncthreads();
    for (uint32_t off = PSIS_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) tm.red[t] = tm.red[t + off] > tm.red[t] ? tm.red[t + off] : tm.red[t];
        __syncthreads();
    }
    return tm.red[0];
#else
    double a = floor_;
    for (uint32_t i = 0; i < n; ++i) { const double v = f(i); a = v > a ? v : a; }
    (void)tm;
    return a;
#endif
}

// f(i) for every i < n, each by one lane; what f stores is visible to every lane afterwards
template <class F>
BPM_PW_HD void psis_each(uint32_t n, F f) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (uint32_t i = threadIdx.x; i < n; i += PSIS_THREADS) f(i);
    __syncthreads();
#else
    for (uint32_t i = 0; i < n; ++i) f(i);
#endif
}

BPM_PW_HD double psis_gpinv(double p, double k, double sigma) {
    if (!(sigma > 0.0)) return NAN;
    const double q = log1p(-p);
    return (fabs(k) < DBL_EPSILON ? -q : expm1(-k * q) / k) * sigma;
}

struct PsisResult {
    double k, sigma, elpd;
    uint64_t tail_len;
};

// sorted: the n_kept >= 1 kept values, ascending; (n_b, m_b, s_b): the body (n_b >= 1); ws: psis_work(n_kept) doubles; smoothed (may be null): takes
// the tail's n log weights lw_j in ascending order of the ratio.  Every lane of the team calls it and gets the same result.
BPM_PW_HD PsisResult psis_datum(const PsisTeam& tm, const double* sorted, uint32_t n_kept, uint64_t n_b, double m_b, double s_b, double* ws, double* smoothed) {
    PsisResult o;
    const double l0 = sorted[0], c = sorted[n_kept - 1];
    uint32_t n = n_kept;
    while (n > 0 && !(sorted[n - 1] < c)) --n;      // (ties with the cutoff are few: every lane scans them)
    o.tail_len = n;
    o.k = INFINITY;
    o.sigma = NAN;
    const double lmin = log(DBL_MIN), xc = l0 - c;
    const double ec = exp(xc > lmin ? xc : lmin);
    double* const y = ws;
    bool smooth = false;
    if (n > 4) {
        const uint32_t m = 30u + (uint32_t)floor(sqrt((double)n));
        double* const b = ws + n_kept;
        double* const L = b + m;
        double* const w = L + m;
        psis_barrier();      // (the work space is free: a previous datum of this team is done)
        psis_each(n, [=](uint32_t j) { y[j] = exp(l0 - sorted[n - 1 - j]) - ec; });
        const double yq = y[(uint32_t)floor((double)n / 4.0 + 0.5) - 1u], yn = y[n - 1];
        const double dn = (double)n;
        for (uint32_t j = 0; j < m; ++j) {
            const double bj = (1.0 - sqrt((double)m / ((double)j + 0.5))) / (3.0 * yq) + 1.0 / yn;
            const double kj = psis_sum(tm, n, [=](uint32_t i) { return log1p(-bj * y[i]); }) / dn;
            if (psis_lane0()) { b[j] = bj; L[j] = dn * (log(-(bj / kj)) - kj - 1.0); }
        }
        psis_barrier();
        psis_each(m, [=](uint32_t j) {
            double t = 0.0;
            for (uint32_t i = 0; i < m; ++i) t += exp(L[i] - L[j]);
            w[j] = 1.0 / t;
        });
        const double cut = 10.0 * DBL_EPSILON;
        double W = 0.0, bp = 0.0;
        for (uint32_t j = 0; j < m; ++j) if (w[j] >= cut) W += w[j];
        for (uint32_t j = 0; j < m; ++j) if (w[j] >= cut) bp += b[j] * (w[j] / W);
        double k = psis_sum(tm, n, [=](uint32_t i) { return log1p(-bp * y[i]); }) / dn;
        o.sigma = -k / bp;
        k = (dn * k + 5.0) / (dn + 10.0);
        o.k = k;
        smooth = k - k == 0.0;      // finite
    }
    double* const lw = ws;      // (y is done with)
    const double k = o.k, sigma = o.sigma, dn = (double)n;
    psis_barrier();
    psis_each(n, [=](uint32_t j) {
        double v = l0 - sorted[n - 1 - j];
        if (smooth) {
            v = log(psis_gpinv(((double)j + 0.5) / dn, k, sigma) + ec);
            v = v > 0.0 ? 0.0 : v;
        }
        lw[j] = v;
        if (smoothed) smoothed[j] = v;
    });
    const double bm = m_b + l0;
    const double A = psis_max(tm, n, l0, [=](uint32_t j) { return sorted[n - 1 - j] + lw[j]; });
    const double B = psis_max(tm, n, bm, [=](uint32_t j) { return lw[j]; });
    const double num = (double)n_b * exp(l0 - A) + psis_sum(tm, n, [=](uint32_t j) { return exp((sorted[n - 1 - j] + lw[j]) - A); });
    const double den = s_b * exp(bm - B) + psis_sum(tm, n, [=](uint32_t j) { return exp(lw[j] - B); });
    o.elpd = (A + log(num)) - (B + log(den));
    return o;
}

#if defined(__HIPCC__)
BPM_PW_HD double psis_key_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// sorted keys (n_cols columns of k_max, ascending, pointwise_tail.h's key) -> the same words as doubles, in place, and cut[q] = the cutoff of column
// q: its largest kept value; NaN for a column without a kept value or with a value that was not finite (stage B then counts no row)
__global__ __launch_bounds__(PSIS_THREADS) void pw_tail_values_kernel(unsigned long long* keys, uint32_t k_max, uint64_t n_cols, const uint32_t* n_kept, const uint32_t* n_bad,
                                                                      double* cut) {
    const uint64_t q = blockIdx.x;
    double* v = reinterpret_cast<double*>(keys) + q * k_max;
    const unsigned long long* kq = keys + q * k_max;
    const uint32_t n = n_kept[q];
    for (uint32_t j = threadIdx.x; j < k_max; j += PSIS_THREADS) {
        const unsigned long long key = kq[j];      // (read and written by the same lane)
        v[j] = j < n ? psis_key_value(key) : __longlong_as_double(0x7FF8000000000000ll);
    }
    __syncthreads();
    if (threadIdx.x == 0) cut[q] = (n > 0 && n_bad[q] == 0u) ? v[n - 1] : __longlong_as_double(0x7FF8000000000000ll);
}

// A workgroup per column q (datum i0 + q, q < n_live): folds stage B's parts in part order, fits, finishes, and stores the datum's record
// (field f at out[f * n_data + i0 + q]).  body: [3][parts * n_cols] as bpm_pointwise_body leaves it; ws: ws_stride doubles per column.
__global__ __launch_bounds__(PSIS_THREADS) void pw_psis_kernel(const double* __restrict__ tails, uint32_t k_max, uint64_t n_cols, const uint32_t* __restrict__ n_kept,
                                                               const uint32_t* __restrict__ n_bad, const double* __restrict__ body, uint32_t parts, double* ws,
                                                               uint64_t ws_stride, uint64_t i0, uint64_t n_data, double* out) {
    __shared__ double red[PSIS_THREADS];
    const uint64_t q = blockIdx.x, i = i0 + q;
    const uint64_t n_rec = (uint64_t)parts * n_cols;
    const unsigned long long* bu = reinterpret_cast<const unsigned long long*>(body);
    unsigned long long nb = 0ull;
    double mb = 0.0, sb = 0.0;
    for (uint32_t p = 0; p < parts; ++p) {
        const uint64_t j = (uint64_t)p * n_cols + q;
        const unsigned long long nn = bu[j];
        pw_merge_lse(nb, mb, sb, nn, body[n_rec + j], body[2 * n_rec + j]);
        nb += nn;
    }
    const uint32_t n = n_kept[q];
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    PsisResult r;
    r.k = nan; r.sigma = nan; r.elpd = nan; r.tail_len = 0;
    if (n > 0 && n_bad[q] == 0u && nb > 0ull) {
        PsisTeam tm;
        tm.red = red;
        r = psis_datum(tm, tails + q * k_max, n, nb, mb, sb, ws + q * ws_stride, nullptr);
    }
    if (threadIdx.x != 0) return;
    unsigned long long* ou = reinterpret_cast<unsigned long long*>(out);
    out[LOO_ELPD * n_data + i] = r.elpd;
    out[LOO_K * n_data + i] = r.k;
    out[LOO_SIGMA * n_data + i] = r.sigma;
    ou[LOO_TAIL_LEN * n_data + i] = r.tail_len;
    ou[LOO_KEPT * n_data + i] = n;
    ou[LOO_BODY_N * n_data + i] = nb;
    out[LOO_BODY_M * n_data + i] = mb;
    out[LOO_BODY_S * n_data + i] = sb;
}
#endif

}  // namespace BPM_VARIANT_NS
}  // namespace bpm
