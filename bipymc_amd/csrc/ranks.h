// Pooled ranks of the resident history (bpm_rank_history): the one transform of a history that is no function of one sample, and what the
// rank-normalized split-R-hat and the bulk / tail ESS of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021) are taken over (no
// counterpart in the reference, whose scripts stop at param_est's mean and standard deviation).  bipymc_amd/rank_diagnostics.py drives the
// fills and finishes the statistics with the split R-hat / ESS the project already has (diagnostics.h, diagnostics.py).
//
// The window is the split rows of history rows [g_lo, g_hi): with n = (g_hi - g_lo) / 2, split row t < n is history row g_lo + t and split
// row t >= n is history row g_hi - 2n + t (an odd window drops its middle row).  Element e = t * n_local + i (split row t, chain i), e < S =
// 2 n n_local, holds its coordinates at H[rk_src_row(e) * ld + k]; the destination holds element e at D[e * ld + k]: a history of 2n rows.
//
//   rk_keys_kernel       grid (column tiles of kw, nby).  Lane = a * kw + kk reads coordinate k0 + blockIdx.x * kw + kk of the elements
//                        blockIdx.y * cpw + a, step nby * cpw (hs_range_kernel's layout: kw contiguous doubles of a row per group of lanes),
//                        RK_UNR loads in flight, and writes keys[(k - k0) * S + e]: the order-preserving key (qs_key) of x + 0.0 (-0.0 and
//                        +0.0 become one key) or, folded, of |x - c[k]|.  Column-major: one segment of S keys per column for the sort.
//   (the sort)           a segmented radix sort of the batch, one segment per column, keys only, on the caller's stream (sampler.hip).
//   rk_pick_kernel       order statistics: out[j * dim + k] = the value of the pos[j]-th smallest key of column k.
//   rk_score_kernel      the same lanes as rk_keys_kernel.  Per element and column: lo = how many keys of the sorted column are smaller
//                        and hi = how many are not larger (two branch-free bisections, RK_UNR elements side by side: every lane makes the
//                        same ceil(log2 S) steps), so the average rank is r = (lo + hi + 1) / 2 -- ties share the mean of their ranks -- with no
//                        index payload in the sort, no run detection and no scatter.  A half-integer below 2^32: exact in a double.
//                        RK_RANK / RK_RANK_FOLDED store r, RK_Z / RK_Z_FOLDED normcdfinv((r - 3/8) / (S + 1/4)).  A column whose largest key is the NaN
//                        key holds a NaN: every element of it is written as NaN.  Stores go to D row-major, kw contiguous doubles per group
//                        of lanes; the lane of the last coordinate also writes the padding column of an odd dim as 0.
//   rk_indicator_kernel  D[e * ld + k] = x <= c[k] ? 1 : 0 (a NaN on either side: 0), or with RK_SQDEV (x - c[k]) * (x - c[k]) -- two IEEE
//                        operations, NumPy's (x - c) ** 2 -- flat over the S * ld elements, the padding column as 0; no sort.
//
// The highest-density interval (bpm_hdi) is read off the same sorted batch: with m = min(floor(p S), S - 1), the first i of [0, S - m) whose
// width w[i] = s[i + m] - s[i] is NaN (inf - inf) if one is, else the first of the smallest width (np.argmin's rule), gives (s[i], s[i + m]).
//   rk_hdi_kernel        grid (column of the batch, part, probability).  A part owns a contiguous range of i, the lanes strided inside it:
//                        col[i] and col[i + m] are two coalesced streams, RK_UNR pairs of 8-byte loads in flight per lane.  Keys are
//                        decoded (hs_unkey) and subtracted in f64.  A lane keeps one candidate (width, index), ordered by (width is NaN
//                        first, smaller width, smaller index): a total order, so neither the lanes' stride nor the order of a reduction
//                        shows in the result.  Candidates meet by shuffles within a wavefront, then in LDS across the workgroup's
//                        wavefronts in wavefront order; one partial per (probability, column, part), no atomics.
//   rk_hdi_final_kernel  one lane per (probability, column): folds the parts in index order and writes lo, hi from the sorted column
//                        (NaN, NaN for a column whose largest key is the NaN key); the lanes of probability 0 also count the column's NaN keys.
// The window of either: the split rows above, or -- e0 > 0, n = every history row -- the contiguous elements from e0 on: param_est's
// selection, super-chain rows >= n_burn with a partial first generation.
// Every index is computed in 64 bits; S < 2^31 and batch * S < 2^31 (the sort's 32-bit offsets) are the host's checks.
#pragma once
#include "kernels.h"
#include "quantiles.h"
#include "histograms.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {      // (philox.h: one kernel-symbol namespace per build variant)

constexpr int RK_THREADS = 256;
constexpr int RK_UNR = 4;              // independent row loads (rk_keys_kernel) / searches (rk_score_kernel) in flight per lane
constexpr int RK_MAX_PROB = 8;         // probabilities of one bpm_hdi call
enum : int32_t { RK_RANK = 0, RK_Z = 1, RK_Z_FOLDED = 2, RK_INDICATOR = 3, RK_RANK_FOLDED = 4, RK_SQDEV = 5 };
__host__ __device__ constexpr bool rk_folded(int32_t kind) { return kind == RK_Z_FOLDED || kind == RK_RANK_FOLDED; }

// the window of a fill, by value in the kernels' arguments
struct RkWindow {
    uint64_t g_lo;       // history row of split row 0
    uint64_t g_up;       // history row of split row n: g_hi - n
    uint64_t n;          // rows per half
    uint64_t n_local;
    uint64_t S;          // 2 n n_local
    uint64_t e0;         // the window's first element (0: whole rows; param_est's window starts inside a generation: g_lo = 0, n = every row, S counted from e0)
};

// element e -> its row of the source history (in rows of ld doubles)
__device__ __forceinline__ uint64_t rk_src_row(const RkWindow& w, uint64_t e) {
    e += w.e0;
    const uint64_t t = e / w.n_local, i = e - t * w.n_local;
    return (t < w.n ? w.g_lo + t : w.g_up + (t - w.n)) * w.n_local + i;
}

__device__ __forceinline__ uint64_t rk_key_of(double x, bool folded, double c) {
    return qs_key(folded ? fabs(x - c) : x + 0.0);
}

// keys: [bc][S]; columns [k0, k0 + bc) of H.  c: [dim] centres (read only when folded)
__global__ __launch_bounds__(RK_THREADS) void rk_keys_kernel(const double* __restrict__ H, uint32_t ld, RkWindow w, uint32_t k0, uint32_t bc, uint32_t kw,
                                                             uint32_t folded, const double* __restrict__ c, unsigned long long* __restrict__ keys) {
    const uint32_t cpw = RK_THREADS / kw, a = threadIdx.x / kw, kk = blockIdx.x * kw + threadIdx.x % kw;
    if (a >= cpw || kk >= bc) return;
    const uint32_t k = k0 + kk;
    const double ck = folded ? c[k] : 0.0;
    unsigned long long* col = keys + (uint64_t)kk * w.S;
    const uint64_t step = (uint64_t)gridDim.y * cpw;
    for (uint64_t e = (uint64_t)blockIdx.y * cpw + a; e < w.S; e += step * RK_UNR) {
        double v[RK_UNR];
#pragma unroll
        for (int u = 0; u < RK_UNR; ++u) {
            const uint64_t ee = e + (uint64_t)u * step;
            v[u] = 0.0;
            if (ee < w.S) v[u] = H[rk_src_row(w, ee) * ld + k];
        }
#pragma unroll
        for (int u = 0; u < RK_UNR; ++u) {
            const uint64_t ee = e + (uint64_t)u * step;
            if (ee < w.S) col[ee] = rk_key_of(v[u], folded != 0u, ck);
        }
    }
}

// sorted: [bc][S] ascending; out[j * dim + k0 + kk] = the value of key pos[j] of column kk (pos[j] < S: the host's check)
__global__ __launch_bounds__(RK_THREADS) void rk_pick_kernel(const unsigned long long* __restrict__ sorted, uint64_t S, uint32_t k0, uint32_t bc, uint32_t dim,
                                                             const unsigned long long* __restrict__ pos, uint32_t n_pos, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * RK_THREADS + threadIdx.x;
    if (i >= n_pos * bc) return;
    const uint32_t j = i / bc, kk = i - j * bc;
    out[(uint64_t)j * dim + k0 + kk] = hs_unkey(sorted[(uint64_t)kk * S + pos[j]]);
}

// RK_UNR searches side by side: lo[u] = how many keys of col[0 .. S) are smaller than key[u], hi[u] = how many are not larger.  Branch-free
// bisection: every lane of every wavefront makes the same ceil(log2 S) steps, each with 2 RK_UNR independent loads in flight.
__device__ __forceinline__ void rk_bounds(const unsigned long long* __restrict__ col, uint32_t S, const unsigned long long (&key)[RK_UNR], uint32_t (&lo)[RK_UNR],
                                          uint32_t (&hi)[RK_UNR]) {
#pragma unroll
    for (int u = 0; u < RK_UNR; ++u) lo[u] = hi[u] = 0u;
    uint32_t len = S;                                // the answer lies in [base, base + len]
    while (len > 1u) {
        const uint32_t half = len >> 1;
        unsigned long long a[RK_UNR], b[RK_UNR];
#pragma unroll
        for (int u = 0; u < RK_UNR; ++u) {
            a[u] = col[lo[u] + half - 1u];
            b[u] = col[hi[u] + half - 1u];
        }
#pragma unroll
        for (int u = 0; u < RK_UNR; ++u) {
            lo[u] += a[u] < key[u] ? half : 0u;
            hi[u] += b[u] <= key[u] ? half : 0u;
        }
        len -= half;
    }
#pragma unroll
    for (int u = 0; u < RK_UNR; ++u) {
        lo[u] += col[lo[u]] < key[u] ? 1u : 0u;
        hi[u] += col[hi[u]] <= key[u] ? 1u : 0u;
    }
}

// one copy of normcdfinv in the kernel: inlined at each of the RK_UNR places it costs rk_score_kernel 256 + 190 registers and all but one
// wavefront per SIMD, and it is the bisection's loads that need the occupancy
__device__ __noinline__ double rk_normal_score(double p) { return normcdfinv(p); }

// D: the destination history, element e at D[e * ld + k]; sorted: [bc][S] the batch's sorted keys
__global__ __launch_bounds__(RK_THREADS) void rk_score_kernel(const double* __restrict__ H, uint32_t ld, uint32_t dim, RkWindow w, uint32_t k0, uint32_t bc,
                                                              uint32_t kw, int32_t kind, const double* __restrict__ c,
                                                              const unsigned long long* __restrict__ sorted, double* __restrict__ D) {
    const uint32_t cpw = RK_THREADS / kw, a = threadIdx.x / kw, kk = blockIdx.x * kw + threadIdx.x % kw;
    if (a >= cpw || kk >= bc) return;
    const uint32_t k = k0 + kk;
    const bool folded = rk_folded(kind), to_z = kind == RK_Z || kind == RK_Z_FOLDED;
    const double ck = folded ? c[k] : 0.0;
    const unsigned long long* col = sorted + (uint64_t)kk * w.S;
    const uint32_t S = (uint32_t)w.S;
    const bool has_nan = col[S - 1u] == ~0ull;
    const bool pad = k + 1u == dim && dim < ld;      // this lane also owns the padding column
    const double denom = (double)S + 0.25;
    const uint64_t step = (uint64_t)gridDim.y * cpw;
    for (uint64_t e = (uint64_t)blockIdx.y * cpw + a; e < w.S; e += step * RK_UNR) {
        unsigned long long key[RK_UNR];
        uint32_t lo[RK_UNR], hi[RK_UNR];
#pragma unroll
        for (int u = 0; u < RK_UNR; ++u) {
            const uint64_t ee = e + (uint64_t)u * step;
            key[u] = rk_key_of(H[rk_src_row(w, ee < w.S ? ee : e) * ld + k], folded, ck);      // (beyond the window: element e again, not stored)
        }
        if (!has_nan) rk_bounds(col, S, key, lo, hi);
#pragma unroll
        for (int u = 0; u < RK_UNR; ++u) {
            const uint64_t ee = e + (uint64_t)u * step;
            if (ee >= w.S) break;
            double r = __longlong_as_double(0x7FF8000000000000ll);
            if (!has_nan) {
                r = ((double)lo[u] + (double)hi[u] + 1.0) * 0.5;
                if (to_z) r = rk_normal_score((r - 0.375) / denom);
            }
            D[ee * ld + k] = r;
            if (pad) D[ee * ld + dim] = 0.0;
        }
    }
}

// flat over the S * ld elements of D; kind RK_INDICATOR or RK_SQDEV
__global__ __launch_bounds__(RK_THREADS) void rk_indicator_kernel(const double* __restrict__ H, uint32_t ld, uint32_t dim, RkWindow w, int32_t kind,
                                                                  const double* __restrict__ c, double* __restrict__ D) {
    const uint64_t total = w.S * ld;
    for (uint64_t j = (uint64_t)blockIdx.x * RK_THREADS + threadIdx.x; j < total; j += (uint64_t)gridDim.x * RK_THREADS) {
        const uint64_t e = j / ld;
        const uint32_t k = (uint32_t)(j - e * ld);
        double v = 0.0;
        if (k < dim) {
            const double x = H[rk_src_row(w, e) * ld + k], ck = c[k];
            if (kind == RK_SQDEV) {
                const double dx = x - ck;
                v = dx * dx;
            } else {
                v = x <= ck ? 1.0 : 0.0;
            }
        }
        D[j] = v;
    }
}

// ---- the highest-density interval over sorted columns ------------------------------------------------------------------------------------
// the offsets m of a call's probabilities, by value in the kernels' arguments
struct RkHdiOffsets {
    uint64_t m[RK_MAX_PROB];
};
// a candidate: the width and its index (RK_HDI_NONE: none yet, beaten by every index).  a before b: a's width is NaN and b's is not; both or
// neither NaN: the smaller width (not compared when NaN), then the smaller index
constexpr uint64_t RK_HDI_NONE = ~0ull;
__device__ __forceinline__ bool rk_hdi_before(double wa, uint64_t ia, double wb, uint64_t ib) {
    const bool na = wa != wa, nb = wb != wb;
    if (na != nb) return na;
    if (!na && wa != wb) return wa < wb;
    return ia < ib;
}

// sorted: [bc][S] ascending; part_w, part_i: [n_prob][bc][parts]
__global__ __launch_bounds__(RK_THREADS) void rk_hdi_kernel(const unsigned long long* __restrict__ sorted, uint64_t S, uint32_t bc, RkHdiOffsets off,
                                                            double* __restrict__ part_w, unsigned long long* __restrict__ part_i) {
    __shared__ double s_w[RK_THREADS / 64];
    __shared__ unsigned long long s_i[RK_THREADS / 64];
    const uint32_t kk = blockIdx.x, part = blockIdx.y, parts = gridDim.y, j = blockIdx.z;
    const unsigned long long* col = sorted + (uint64_t)kk * S;
    const uint64_t m = off.m[j], count = S - m;                       // (m <= S - 1: the host's clamp)
    const uint64_t chunk = (count + parts - 1) / parts;
    const uint64_t i_lo = (uint64_t)part * chunk < count ? (uint64_t)part * chunk : count;
    const uint64_t i_hi = i_lo + chunk < count ? i_lo + chunk : count;
    double bw = __longlong_as_double(0x7FF0000000000000ll);
    uint64_t bi = RK_HDI_NONE;
    if (col[S - 1u] != ~0ull) {                                       // (a column with a NaN is (NaN, NaN) whatever the widths)
        for (uint64_t i = i_lo + threadIdx.x; i < i_hi; i += (uint64_t)RK_THREADS * RK_UNR) {
            unsigned long long a[RK_UNR], b[RK_UNR];
#pragma unroll
            for (int u = 0; u < RK_UNR; ++u) {
                const uint64_t ii = i + (uint64_t)u * RK_THREADS;
                const uint64_t at = ii < i_hi ? ii : i;               // (beyond the part: index i again, not considered)
                a[u] = col[at];
                b[u] = col[at + m];
            }
#pragma unroll
            for (int u = 0; u < RK_UNR; ++u) {
                const uint64_t ii = i + (uint64_t)u * RK_THREADS;
                const double wd = hs_unkey(b[u]) - hs_unkey(a[u]);
                if (ii < i_hi && rk_hdi_before(wd, ii, bw, bi)) { bw = wd; bi = ii; }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ow = __shfl_xor(bw, d, 64);
        const uint64_t oi = (uint64_t)__shfl_xor((unsigned long long)bi, d, 64);
        if (rk_hdi_before(ow, oi, bw, bi)) { bw = ow; bi = oi; }
    }
    if ((threadIdx.x & 63u) == 0u) { s_w[threadIdx.x >> 6] = bw; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t v = 1; v < RK_THREADS / 64; ++v)
            if (rk_hdi_before(s_w[v], s_i[v], bw, bi)) { bw = s_w[v]; bi = s_i[v]; }
        const uint64_t o = ((uint64_t)j * bc + kk) * parts + part;
        part_w[o] = bw;
        part_i[o] = bi;
    }
}

// lo, hi: [n_prob][dim]; n_nan: [dim]
__global__ __launch_bounds__(RK_THREADS) void rk_hdi_final_kernel(const unsigned long long* __restrict__ sorted, uint64_t S, uint32_t k0, uint32_t bc, uint32_t dim,
                                                                  uint32_t n_prob, uint32_t parts, RkHdiOffsets off, const double* __restrict__ part_w,
                                                                  const unsigned long long* __restrict__ part_i, double* __restrict__ lo,
                                                                  double* __restrict__ hi, long long* __restrict__ n_nan) {
    const uint32_t t = blockIdx.x * RK_THREADS + threadIdx.x;
    if (t >= n_prob * bc) return;
    const uint32_t j = t / bc, kk = t - j * bc;
    const unsigned long long* col = sorted + (uint64_t)kk * S;
    const bool has_nan = col[S - 1u] == ~0ull;
    double a = __longlong_as_double(0x7FF8000000000000ll), b = a;
    if (!has_nan) {
        const uint64_t o = ((uint64_t)j * bc + kk) * parts;
        double bw = part_w[o];
        uint64_t bi = part_i[o];
        for (uint32_t p = 1; p < parts; ++p)
            if (rk_hdi_before(part_w[o + p], part_i[o + p], bw, bi)) { bw = part_w[o + p]; bi = part_i[o + p]; }
        if (bi < S - off.m[j]) {                                      // (every column has one index at least: part 0 is never empty)
            a = hs_unkey(col[bi]);
            b = hs_unkey(col[bi + off.m[j]]);
        }
    }
    lo[(uint64_t)j * dim + k0 + kk] = a;
    hi[(uint64_t)j * dim + k0 + kk] = b;
    if (j == 0u) {
        uint64_t first = 0, len = S;                                  // the first NaN key: how many keys are smaller than ~0
        while (len > 0u) {
            const uint64_t half = len >> 1;
            if (col[first + half] != ~0ull) { first += half + 1u; len -= half + 1u; } else { len = half; }
        }
        n_nan[k0 + kk] = (long long)(S - first);
    }
}

}  // inline namespace BPM_VARIANT_NS
}  // namespace bpm
