// Marginal and pairwise histograms of the resident history: the counts behind the reference's corner plot (corner.corner over the gathered
// super chain, mc_plot/mc_plot.py:16-29: a 1-D histogram per parameter, a 2-D histogram per pair).  The host (bipymc_amd/histograms.py)
// applies NumPy's range rules, builds the edges with np.linspace and merges the ranks; the device finds the range and counts.
//
// The window is a contiguous range [r_lo, r_hi) of local super-chain rows; row r holds its coordinates at H[r * ld + k], k < ld.
//
// Binning rule (NumPy's, np.histogram and np.histogram2d alike): with edges e[0..nb], bin i counts e[i] <= x < e[i + 1], the last bin also
// x == e[nb]; NaN and values outside [e[0], e[nb]] are counted nowhere.  hs_bin guesses i = (x - e[0]) * (nb / (e[nb] - e[0])) and corrects
// the guess against the stored edges (one step either way, a binary search beyond that), so the inequality holds exactly whatever the
// rounding of the guess: the result is the largest i <= nb - 1 with e[i] <= x.
//
//   hs_range_kernel      grid (column tiles of HS_THREADS, nby).  Lane = a * kw + kk reads coordinate k0 + kk of the rows blockIdx.y * cpw + a,
//                        step nby * cpw (cpw = HS_THREADS / kw rows side by side: kw contiguous doubles of a row per group of lanes),
//                        HS_UNR loads in flight.  Per lane: min and max of the values that are not NaN, how many are NaN, how many
//                        infinite.  The cpw lanes of a coordinate are merged in LDS in a fixed order; workgroups merge through integer
//                        atomics on order-preserving keys (qs_key: unsigned order = numeric order), so no floating-point atomic and no
//                        dependence on the order of the workgroups.  out: [min keys ld | max keys ld | NaN counts ld | inf counts ld].
//   hs_marginal_kernel   grid (n_tiles, nby).  A slot is one requested coordinate with its nb + 1 edges; a tile is kw consecutive slots.  A
//                        workgroup keeps the tile's edges and `rep` copies of its uint32 histograms in LDS (the copy is chosen by the
//                        lane's row, so rows that fall into one peaked bin do not all meet at one address), walks the rows as above and
//                        flushes to the global uint64 counters by integer atomics.  The tile index varies fastest: workgroups that read
//                        the same rows run side by side and share their cache lines (quantiles.h).
//   hs_pair_kernel       grid (n_tiles, nby).  A tile is np pairs over nu distinct slots.  Per chunk of cpw1 * HS_UNR rows: phase 1, lane
//                        (row, slot) computes the slot's bin of the row once and stores it as a byte in LDS; phase 2, lane (row, pair)
//                        reads the two bytes and adds 1 to cell [bin a][bin b] of the pair's uint32 histogram in LDS (pairs vary fastest
//                        across lanes: the lanes of one instruction hit different histograms).  Flushed like the marginals.
// Counts that leave a workgroup are 64-bit; a workgroup sees fewer than 2^31 rows (the host sizes nby so).
#pragma once
#include "kernels.h"
#include "quantiles.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {      // (philox.h: one kernel-symbol namespace per build variant)

constexpr int HS_THREADS = 256;
constexpr int HS_UNR = 4;                      // independent row loads in flight per lane
constexpr int HS_MAX_BINS = 1024;
constexpr int HS_MAX_BINS2D = 64;
constexpr uint32_t HS_NONE = 0xFFFFFFFFu;      // hs_bin: counted nowhere
constexpr uint32_t HS_NONE8 = 255u;            // the same as a byte (bins2d <= 64)

__device__ __forceinline__ double hs_unkey(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// e: nb + 1 non-decreasing edges (in LDS); scale = nb / (e[nb] - e[0]) (any value, also inf, 0 or NaN: the edges decide)
__device__ __forceinline__ uint32_t hs_bin(double x, const double* e, uint32_t nb, double e0, double eN, double scale) {
    if (!(x >= e0 && x <= eN)) return HS_NONE;
    const double t = (x - e0) * scale;
    uint32_t i = t >= 0.0 ? (t < (double)nb ? (uint32_t)t : nb - 1u) : 0u;
    if (x < e[i]) {                                   // (i > 0 here: x >= e[0])
        if (x >= e[i - 1u]) return i - 1u;
    } else if (i + 1u >= nb || x < e[i + 1u]) {
        return i;
    } else if (i + 2u >= nb || x < e[i + 2u]) {
        return i + 1u;
    }
    uint32_t lo = 0u, hi = nb - 1u;                   // the largest i with e[i] <= x
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (e[mid] <= x) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// out: [min keys ld | max keys ld | NaN counts ld | inf counts ld], set by the caller to key(+inf), key(-inf), 0, 0
__global__ __launch_bounds__(HS_THREADS) void hs_range_kernel(const double* __restrict__ H, uint32_t ld, uint64_t r_lo, uint64_t r_hi, uint32_t kw,
                                                              unsigned long long* __restrict__ out) {
    __shared__ double s_mn[HS_THREADS], s_mx[HS_THREADS];
    __shared__ uint32_t s_nan[HS_THREADS], s_inf[HS_THREADS];
    const uint32_t cpw = HS_THREADS / kw, a = threadIdx.x / kw, kk = threadIdx.x % kw;
    const uint32_t k = blockIdx.x * kw + kk;
    double mn = __longlong_as_double(0x7FF0000000000000ll), mx = -mn;
    uint32_t n_nan = 0u, n_inf = 0u;
    if (a < cpw && k < ld) {
        const uint64_t step = (uint64_t)gridDim.y * cpw;
        for (uint64_t r = r_lo + (uint64_t)blockIdx.y * cpw + a; r < r_hi; r += step * HS_UNR) {
            double v[HS_UNR];
#pragma unroll
            for (int u = 0; u < HS_UNR; ++u) {
                const uint64_t rr = r + (uint64_t)u * step;
                v[u] = 0.0;
                if (rr < r_hi) v[u] = H[rr * ld + k];
            }
#pragma unroll
            for (int u = 0; u < HS_UNR; ++u) {
                if (r + (uint64_t)u * step >= r_hi) break;
                const double x = v[u];
                if (x != x) {
                    ++n_nan;
                } else {
                    mn = x < mn ? x : mn;
                    mx = x > mx ? x : mx;
                    if (x - x != 0.0) ++n_inf;
                }
            }
        }
    }
    s_mn[threadIdx.x] = mn; s_mx[threadIdx.x] = mx; s_nan[threadIdx.x] = n_nan; s_inf[threadIdx.x] = n_inf;
    __syncthreads();
    if (a == 0u && k < ld) {
        for (uint32_t j = 1; j < cpw; ++j) {
            const uint32_t o = j * kw + kk;
            mn = s_mn[o] < mn ? s_mn[o] : mn;
            mx = s_mx[o] > mx ? s_mx[o] : mx;
            n_nan += s_nan[o];
            n_inf += s_inf[o];
        }
        const unsigned long long kmn = qs_key(mn), kmx = qs_key(mx);
        if (kmn < out[k]) atomicMin(&out[k], kmn);                     // (a plain read first: most workgroups improve nothing)
        if (kmx > out[ld + k]) atomicMax(&out[ld + k], kmx);
        if (n_nan) atomicAdd(&out[2u * ld + k], (unsigned long long)n_nan);
        if (n_inf) atomicAdd(&out[3u * ld + k], (unsigned long long)n_inf);
    }
}

// dynamic LDS: [edges kw x (nb + 1) doubles | counts rep x kw x nb uint32].  dims: [m] coordinates; edges: [m][nb + 1]; counts: [m][nb], zeroed
__global__ __launch_bounds__(HS_THREADS) void hs_marginal_kernel(const double* __restrict__ H, uint32_t ld, uint64_t r_lo, uint64_t r_hi,
                                                                 const uint32_t* __restrict__ dims, uint32_t m, uint32_t nb,
                                                                 const double* __restrict__ edges, uint32_t kw, uint32_t rep,
                                                                 unsigned long long* __restrict__ counts) {
    extern __shared__ double hs_lds[];
    double* s_e = hs_lds;
    uint32_t* s_h = reinterpret_cast<uint32_t*>(s_e + kw * (nb + 1u));
    const uint32_t s0 = blockIdx.x * kw;
    const uint32_t ns = m - s0 < kw ? m - s0 : kw;
    for (uint32_t i = threadIdx.x; i < ns * (nb + 1u); i += HS_THREADS) s_e[i] = edges[(uint64_t)s0 * (nb + 1u) + i];
    for (uint32_t i = threadIdx.x; i < rep * kw * nb; i += HS_THREADS) s_h[i] = 0u;
    const uint32_t cpw = HS_THREADS / kw, a = threadIdx.x / kw, kk = threadIdx.x % kw;
    __syncthreads();
    if (a < cpw && kk < ns) {
        const uint32_t k = dims[s0 + kk];
        const double* e = s_e + kk * (nb + 1u);
        const double e0 = e[0], eN = e[nb], scale = (double)nb / (eN - e0);
        uint32_t* h = s_h + ((a % rep) * kw + kk) * nb;
        const uint64_t step = (uint64_t)gridDim.y * cpw;
        for (uint64_t r = r_lo + (uint64_t)blockIdx.y * cpw + a; r < r_hi; r += step * HS_UNR) {
            double v[HS_UNR];
#pragma unroll
            for (int u = 0; u < HS_UNR; ++u) {
                const uint64_t rr = r + (uint64_t)u * step;
                v[u] = 0.0;
                if (rr < r_hi) v[u] = H[rr * ld + k];
            }
#pragma unroll
            for (int u = 0; u < HS_UNR; ++u) {
                if (r + (uint64_t)u * step >= r_hi) break;
                const uint32_t i = hs_bin(v[u], e, nb, e0, eN, scale);
                if (i != HS_NONE) atomicAdd(&h[i], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < ns * nb; i += HS_THREADS) {
        uint32_t c = 0u;
        for (uint32_t q = 0; q < rep; ++q) c += s_h[q * kw * nb + i];
        if (c) atomicAdd(&counts[(uint64_t)s0 * nb + i], (unsigned long long)c);
    }
}

// tiles: [n_tiles] of {first pair, pairs np, first entry of uslot, slots nu}; uslot: the tiles' distinct slots, one list after the other;
// pl: [P] of {index of a, index of b} in the tile's list; dims: [m]; edges: [m][nb + 1]; counts: [P][nb][nb], zeroed.
// dynamic LDS: [edges nu_max x (nb + 1) doubles | counts np_max x nb x nb uint32 | bins HS_THREADS x HS_UNR bytes]
__global__ __launch_bounds__(HS_THREADS) void hs_pair_kernel(const double* __restrict__ H, uint32_t ld, uint64_t r_lo, uint64_t r_hi,
                                                             const uint4* __restrict__ tiles, const uint32_t* __restrict__ uslot,
                                                             const uint2* __restrict__ pl, const uint32_t* __restrict__ dims, uint32_t nb,
                                                             const double* __restrict__ edges, uint32_t nu_max, uint32_t np_max,
                                                             unsigned long long* __restrict__ counts) {
    extern __shared__ double hs_lds[];
    double* s_e = hs_lds;
    uint32_t* s_h = reinterpret_cast<uint32_t*>(s_e + nu_max * (nb + 1u));
    unsigned char* s_bin = reinterpret_cast<unsigned char*>(s_h + np_max * nb * nb);
    const uint4 t = tiles[blockIdx.x];
    const uint32_t p0 = t.x, np = t.y, u0 = t.z, nu = t.w;
    const uint32_t cells = nb * nb;
    for (uint32_t i = threadIdx.x; i < nu * (nb + 1u); i += HS_THREADS) {
        const uint32_t u = i / (nb + 1u);
        s_e[i] = edges[(uint64_t)uslot[u0 + u] * (nb + 1u) + (i - u * (nb + 1u))];
    }
    for (uint32_t i = threadIdx.x; i < np * cells; i += HS_THREADS) s_h[i] = 0u;
    const uint32_t cpw1 = HS_THREADS / nu, a1 = threadIdx.x / nu, u = threadIdx.x % nu;
    const uint32_t cpw2 = HS_THREADS / np, a2 = threadIdx.x / np, p = threadIdx.x % np;
    const uint32_t rc = cpw1 * HS_UNR;                     // rows of a chunk
    const bool on1 = a1 < cpw1, on2 = a2 < cpw2;
    const uint32_t k = dims[uslot[u0 + u]];
    const uint2 ab = pl[p0 + p];
    uint32_t* h = s_h + p * cells;
    __syncthreads();
    const double* e = s_e + u * (nb + 1u);
    const double e0 = e[0], eN = e[nb], scale = (double)nb / (eN - e0);
    for (uint64_t r0 = r_lo + (uint64_t)blockIdx.y * rc; r0 < r_hi; r0 += (uint64_t)gridDim.y * rc) {
        const uint32_t n_row = r_hi - r0 < rc ? (uint32_t)(r_hi - r0) : rc;
        if (on1) {
            double v[HS_UNR];
#pragma unroll
            for (int j = 0; j < HS_UNR; ++j) {
                const uint32_t a = a1 + (uint32_t)j * cpw1;
                v[j] = 0.0;
                if (a < n_row) v[j] = H[(r0 + a) * ld + k];
            }
#pragma unroll
            for (int j = 0; j < HS_UNR; ++j) {
                const uint32_t a = a1 + (uint32_t)j * cpw1;
                if (a < n_row) {
                    const uint32_t i = hs_bin(v[j], e, nb, e0, eN, scale);
                    s_bin[a * nu + u] = (unsigned char)(i == HS_NONE ? HS_NONE8 : i);
                }
            }
        }
        __syncthreads();
        if (on2) {
            for (uint32_t a = a2; a < n_row; a += cpw2) {
                const uint32_t ia = s_bin[a * nu + ab.x], ib = s_bin[a * nu + ab.y];
                if (ia != HS_NONE8 && ib != HS_NONE8) atomicAdd(&h[ia * nb + ib], 1u);
            }
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < np * cells; i += HS_THREADS) {
        const uint32_t c = s_h[i];
        if (c) atomicAdd(&counts[(uint64_t)p0 * cells + i], (unsigned long long)c);
    }
}

}  // inline namespace BPM_VARIANT_NS
}  // namespace bpm
