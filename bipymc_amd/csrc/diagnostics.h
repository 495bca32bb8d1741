// Convergence diagnostics on the resident history (no counterpart in the reference): split-chain R-hat and the autocovariances
// behind the effective sample size (Gelman et al., Bayesian Data Analysis 3rd ed. ch. 11; Geyer 1992; the split-chain form of Stan /
// ArviZ ess(method="mean")).  The definitions, and the host side that finishes them, are in bipymc_amd/diagnostics.py.
//
// The history is generation-major: row g = n_local x ld doubles (chain i, coordinate k at i * ld + k).  A window [g0, g1) of G rows gives
// n = G / 2 draws per half-chain; half 0 = rows [g0, g0 + n), half 1 = rows [g1 - n, g1).  Half-chain j = h * n_local + i.
//
//   diag_split_moments_kernel   one thread per (half, chain, coordinate PAIR): walks the n rows of its half with 16-byte loads, DIAG_UNR in
//                               flight -- the access pattern of moments_partial_kernel (a row's pairs are contiguous across threads) --
//                               and writes the half-chain's mean and M2 (sum of squared deviations), shifted by the half's first value
//   diag_means_final_kernel     per coordinate over the 2 n_local half-chains, in a fixed order: mean of the means, sum of squared
//                               deviations of the means from it (two passes), sum of the half-chain variances (ddof 1)
//   diag_autocov_kernel         sum over half-chains of the un-normalised lag products for DIAG_T lags [t0, t0 + DIAG_T): one lane per
//                               (half-chain, coordinate) column; the last DIAG_T centred values of the lagged stream in a ring of registers
//                               whose slots are compile-time constants (the time loop is unrolled by DIAG_T); per-workgroup partials
//   diag_autocov_final_kernel   the partials in a fixed order, divided by n
//
// No atomics: every result is a fixed-order function of the history and the grid, which depends on the shape only.
// Non-finite values: a coordinate with a NaN or an inf in either half has NaN in every output; no other coordinate sees it
// (tests/test_gpu_diagnostics_edges.py).
#pragma once
#include "kernels.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {      // (philox.h: one kernel-symbol namespace per build variant)

constexpr int DIAG_THREADS = 256;
constexpr int DIAG_UNR = 8;        // independent 16-byte loads in flight per thread (split moments)
// lags per autocovariance launch: 16 accumulators + a 16-slot ring (2 x 32 VGPRs); the compiler hoists the whole unrolled block's loads
// (another 2 x 32), 138 VGPRs in all, 3 waves per SIMD.  32 lags need 256 + spills.
constexpr int DIAG_T = 16;
constexpr int DIAG_B = 8;          // autocovariance: rows loaded ahead per batch (8 of the column, 8 of the lagged column)
constexpr int DIAG_FIN_K = 16;     // diag_autocov_final_kernel: coordinates per workgroup (x 16 slices of the partials)

// grid (ceil(n_pairs / 256), 2): blockIdx.y = half.  mean / m2: [2][n_local][ld].
__global__ __launch_bounds__(DIAG_THREADS) void diag_split_moments_kernel(const double* H, uint64_t row_d, uint64_t n_pairs, uint64_t r_lo0,
                                                                        uint64_t r_lo1, uint32_t n, double* mean, double* m2) {
    const uint64_t p = (uint64_t)blockIdx.x * DIAG_THREADS + threadIdx.x;
    if (p >= n_pairs) return;
    const uint32_t h = blockIdx.y;
    const double2* col = reinterpret_cast<const double2*>(H + (h == 0 ? r_lo0 : r_lo1) * row_d) + p;
    const uint64_t stride = row_d / 2u;      // double2 per row
    const double2 first = col[0];
    const double shx = first.x, shy = first.y;
    double sa0 = 0.0, sa1 = 0.0, sb0 = 0.0, sb1 = 0.0;
    for (uint32_t i = 0; i < n; i += DIAG_UNR) {
        double2 v[DIAG_UNR];
#pragma unroll
        for (int u = 0; u < DIAG_UNR; ++u) {
            v[u] = make_double2(shx, shy);
            if (i + (uint32_t)u < n) v[u] = col[(uint64_t)(i + u) * stride];
        }
#pragma unroll
        for (int u = 0; u < DIAG_UNR; ++u) {
            const double d0 = v[u].x - shx, d1 = v[u].y - shy;
            sa0 += d0; sb0 += d0 * d0;
            sa1 += d1; sb1 += d1 * d1;
        }
    }
    const double inv = 1.0 / (double)n;
    const double m0 = sa0 * inv, m1 = sa1 * inv;
    double2* om = reinterpret_cast<double2*>(mean + h * 2u * n_pairs) + p;
    double2* o2 = reinterpret_cast<double2*>(m2 + h * 2u * n_pairs) + p;
    // A half-chain that holds a NaN or an inf has M2 = NaN (inf - inf at the latest) and, with it, mean = NaN: an inf met after the first row
    // would leave mean = inf, one in the first row NaN.  So M2 is clamped at 0 with a comparison, not with fmax -- fmax(NaN, 0) is 0, a
    // variance of zero for such a half-chain -- and every output of the coordinate is NaN wherever in the half the value lies.
    const double v0 = sb0 - sa0 * m0, v1 = sb1 - sa1 * m1;
    const double nan = __builtin_nan("");
    *om = make_double2(v0 == v0 ? shx + m0 : nan, v1 == v1 ? shy + m1 : nan);
    *o2 = make_double2(v0 < 0.0 ? 0.0 : v0, v1 < 0.0 ? 0.0 : v1);
}

// one workgroup per coordinate k < ld; m_half = 2 n_local half-chains at stride ld.  out: [0, ld) mean of the means, [ld, 2 ld) sum of
// squared deviations of the means, [2 ld, 3 ld) sum of M2 / (n - 1).
__global__ __launch_bounds__(DIAG_THREADS) void diag_means_final_kernel(const double* mean, const double* m2, uint32_t m_half, uint32_t ld,
                                                                      uint32_t n, double* out) {
    __shared__ double s_a[DIAG_THREADS], s_b[DIAG_THREADS];
    const uint32_t k = blockIdx.x;
    double sa = 0.0, sb = 0.0;
    for (uint32_t j = threadIdx.x; j < m_half; j += DIAG_THREADS) {
        sa += mean[(uint64_t)j * ld + k];
        sb += m2[(uint64_t)j * ld + k] / (double)(n - 1u);
    }
    s_a[threadIdx.x] = sa; s_b[threadIdx.x] = sb;
    __syncthreads();
    for (int o = DIAG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s_a[threadIdx.x] += s_a[threadIdx.x + o]; s_b[threadIdx.x] += s_b[threadIdx.x + o]; }
        __syncthreads();
    }
    const double mu = s_a[0] / (double)m_half, sum_var = s_b[0];
    __syncthreads();
    double sd = 0.0;
    for (uint32_t j = threadIdx.x; j < m_half; j += DIAG_THREADS) {
        const double e = mean[(uint64_t)j * ld + k] - mu;
        sd += e * e;
    }
    s_a[threadIdx.x] = sd;
    __syncthreads();
    for (int o = DIAG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_a[threadIdx.x] += s_a[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[k] = mu; out[ld + k] = s_a[0]; out[2u * ld + k] = sum_var; }
}

// grid (nb, n_kt, 2): blockIdx.z = half, blockIdx.y = coordinate tile of kw columns (kw = ld if ld <= 256, else 256); a workgroup holds
// cpw = 256 / kw chains side by side (lane = a * kw + kk) and walks groups of them g = blockIdx.x, blockIdx.x + nb, ...  The row a step
// reads is the same for the whole workgroup (a scalar base), a lane adds its 32-bit column offset.  A lane sums, over its half-chains, for
// lag t0 + u (u < DIAG_T):  sum_{i = t0 + u}^{n - 1} y_i y_{i - t0 - u},  y = x - (the half-chain's mean).  part: [2 nb][DIAG_T][ld].
__global__ __launch_bounds__(DIAG_THREADS) void diag_autocov_kernel(const double* H, uint64_t row_d, uint32_t n_local, uint32_t ld,
                                                                     uint64_t r_lo0, uint64_t r_lo1, uint32_t n, uint32_t t0, const double* mean,
                                                                     uint32_t kw, uint32_t cpw, double* part) {
    __shared__ double red[DIAG_THREADS];
    const uint32_t h = blockIdx.z;
    const uint64_t r_lo = h == 0 ? r_lo0 : r_lo1;
    const uint32_t a = threadIdx.x / kw, kk = threadIdx.x % kw;
    const uint32_t k = blockIdx.y * kw + kk;
    const bool lane_ok = a < cpw && k < ld;
    double acc[DIAG_T];
#pragma unroll
    for (int l = 0; l < DIAG_T; ++l) acc[l] = 0.0;
    for (uint32_t g = blockIdx.x; g * cpw < n_local; g += gridDim.x) {
        const uint32_t i = g * cpw + a;
        const bool ok = lane_ok && i < n_local;
        // a lane without a column loads column 0 (so that the loads stay uniform) and uses none of it: its y AND its ring entries are zero,
        // so it adds exactly zero whatever column 0 holds -- 0 x NaN or 0 x inf would be NaN, and red[] below sums every lane of a coordinate
        const uint32_t off = ok ? i * ld + k : 0u;
        const double mu = mean[(uint64_t)h * n_local * ld + off];
        double ring[DIAG_T];
#pragma unroll
        for (int l = 0; l < DIAG_T; ++l) ring[l] = 0.0;
        // step idx = i0 + s (row of the half, i0 = t0 + a multiple of DIAG_T): ring[s] = y_{idx - t0}; lag t0 + u pairs y_idx with
        // ring[(s - u) mod DIAG_T] = y_{idx - t0 - u} (zero before the half's first row)
        for (uint32_t i0 = t0; i0 < n; i0 += DIAG_T) {
#pragma unroll
            for (int b = 0; b < DIAG_T; b += DIAG_B) {
                double xv[DIAG_B], zv[DIAG_B];
#pragma unroll
                for (int u = 0; u < DIAG_B; ++u) {
                    const uint32_t idx = i0 + (uint32_t)(b + u);
                    xv[u] = mu;
                    zv[u] = mu;
                    if (idx < n) {
                        xv[u] = (H + (r_lo + idx) * row_d)[off];
                        zv[u] = t0 == 0 ? xv[u] : (H + (r_lo + idx - t0) * row_d)[off];
                    }
                }
#pragma unroll
                for (int u = 0; u < DIAG_B; ++u) {
                    const int s = b + u;
                    const double y = ok ? xv[u] - mu : 0.0;
                    ring[s] = ok ? zv[u] - mu : 0.0;
#pragma unroll
                    for (int l = 0; l < DIAG_T; ++l) acc[l] = fma(y, ring[(s - l + DIAG_T) % DIAG_T], acc[l]);
                }
            }
        }
    }
    // per-workgroup partials: the cpw chains of a coordinate in lane order
    const uint64_t wg = (uint64_t)blockIdx.z * gridDim.x + blockIdx.x;
#pragma unroll
    for (int l = 0; l < DIAG_T; ++l) {
        red[threadIdx.x] = acc[l];
        __syncthreads();
        if (a == 0 && k < ld) {
            double sum = red[kk];
            for (uint32_t aa = 1; aa < cpw; ++aa) sum += red[aa * kw + kk];
            part[(wg * DIAG_T + l) * ld + k] = sum;
        }
        __syncthreads();
    }
}

// grid (ceil(ld / DIAG_FIN_K), DIAG_T): lane = slice * DIAG_FIN_K + kk sums the partials b = slice, slice + 16, ... of lag blockIdx.y, the 16
// slices are then added in order.  out: [DIAG_T][ld], divided by n.
__global__ __launch_bounds__(DIAG_THREADS) void diag_autocov_final_kernel(const double* part, uint32_t nb, uint32_t ld, uint32_t n, double* out) {
    constexpr uint32_t SL = DIAG_THREADS / DIAG_FIN_K;
    __shared__ double red[DIAG_THREADS];
    const uint32_t kk = threadIdx.x % DIAG_FIN_K, sl = threadIdx.x / DIAG_FIN_K;
    const uint32_t k = blockIdx.x * DIAG_FIN_K + kk, l = blockIdx.y;
    double sum = 0.0;
    if (k < ld)
        for (uint32_t b = sl; b < nb; b += SL) sum += part[((uint64_t)b * DIAG_T + l) * ld + k];
    red[threadIdx.x] = sum;
    __syncthreads();
    if (sl == 0 && k < ld) {
        for (uint32_t s = 1; s < SL; ++s) sum += red[s * DIAG_FIN_K + kk];
        out[(uint64_t)l * ld + k] = sum / (double)n;
    }
}

}  // inline namespace BPM_VARIANT_NS
}  // namespace bpm
