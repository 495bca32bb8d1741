// Exact posterior quantiles of the resident history (no counterpart on the GPU in the reference, which prints 5/50/95 percentiles of host
// chains, mc_plot/vis_mcmc_chains.py:76): the digit histograms of an MSD radix select over order-preserving 64-bit keys.  The select
// itself, the merge of the ranks and NumPy's interpolation are in bipymc_amd/quantiles.py.
//
// Key of a double x (qs_key): negative -> all bits flipped, otherwise the sign bit set; every NaN -> ~0 (above +inf).  Unsigned order of the
// keys = numeric order of the values, -0.0 just below +0.0.
//
// The window is a contiguous range [r_lo, r_hi) of local super-chain rows r = g * n_local + i (history row g, chain i); row r holds its
// coordinates at H[r * ld + k], k < ld (padding columns k >= dim are never named by a prefix, so never counted).
//
//   qs_histogram_kernel   grid (n_tiles, nby).  A *slot* is one (coordinate, prefix) pair of the request; slots are sorted by coordinate
//                         and cut into tiles of at most QS_SLOTS slots spanning at most QS_SLOTS coordinates (tiles: [n_tiles] of {first
//                         slot, slots, first coordinate, coordinates}).  A workgroup holds the tile's 256-bin uint32 histograms in LDS
//                         (QS_SLOTS KiB) and walks the rows blockIdx.y * cpw + a, step nby * cpw (cpw = 256 / kw rows side by side, lane
//                         = a * kw + kk reads coordinate k0 + kk: kw contiguous doubles of a row per group of lanes), QS_UNR loads in
//                         flight.  A key whose top `bits` bits equal a slot's prefix adds 1 to the slot's bin (key >> (56 - bits)) & 255
//                         (prefixes of one coordinate are distinct, so at most one matches).  The tile dimension varies fastest, so the
//                         workgroups that read one range of rows run side by side and share its cache lines.  Per-workgroup counts go to
//                         the global uint64 histograms by integer atomics: the sums are independent of their order.
#pragma once
#include "kernels.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {      // (philox.h: one kernel-symbol namespace per build variant)

constexpr int QS_THREADS = 256;
constexpr int QS_SLOTS = 32;       // histograms per workgroup: 32 x 256 x 4 B = 32 KiB of LDS, four workgroups per CU
constexpr int QS_UNR = 4;          // independent row loads in flight per lane

__device__ __forceinline__ uint64_t qs_key(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    if (x != x) return ~0ull;
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// hist: [n_prefix][256], n_nan: [n_prefix] (keys of the slot that are NaN), both zeroed by the caller.  bits in {0, 8, ..., 56}.
__global__ __launch_bounds__(QS_THREADS) void qs_histogram_kernel(const double* H, uint32_t ld, uint64_t r_lo, uint64_t r_hi,
                                                                  const uint4* tiles, const uint32_t* pk, const uint64_t* pv, uint32_t bits,
                                                                  unsigned long long* hist, unsigned long long* n_nan) {
    __shared__ uint32_t s_h[QS_SLOTS * 256];
    __shared__ uint32_t s_nan[QS_SLOTS];
    __shared__ uint64_t s_pv[QS_SLOTS];
    const uint4 t = tiles[blockIdx.x];
    const uint32_t p0 = t.x, ns = t.y, k0 = t.z, kw = t.w;
    for (uint32_t i = threadIdx.x; i < (uint32_t)QS_SLOTS * 256u; i += QS_THREADS) s_h[i] = 0u;
    if (threadIdx.x < (uint32_t)QS_SLOTS) {
        s_nan[threadIdx.x] = 0u;
        s_pv[threadIdx.x] = threadIdx.x < ns ? pv[p0 + threadIdx.x] : 0ull;
    }
    const uint32_t cpw = QS_THREADS / kw, a = threadIdx.x / kw, kk = threadIdx.x % kw;
    const uint32_t k = k0 + kk;
    uint32_t s_lo = ns, s_hi = ns;                   // this lane's slots [s_lo, s_hi) of the tile
    for (uint32_t s = 0; s < ns; ++s)
        if (pk[p0 + s] == k) {
            if (s_lo == ns) s_lo = s;
            s_hi = s + 1u;
        }
    __syncthreads();
    if (a < cpw && s_lo < s_hi) {
        const uint32_t dsh = 56u - bits;
        const uint32_t psh = bits == 0u ? 0u : 64u - bits;
        const uint64_t step = (uint64_t)gridDim.y * cpw;
        for (uint64_t r = r_lo + (uint64_t)blockIdx.y * cpw + a; r < r_hi; r += step * QS_UNR) {
            double v[QS_UNR];
#pragma unroll
            for (int u = 0; u < QS_UNR; ++u) {
                const uint64_t rr = r + (uint64_t)u * step;
                v[u] = 0.0;
                if (rr < r_hi) v[u] = H[rr * ld + k];
            }
#pragma unroll
            for (int u = 0; u < QS_UNR; ++u) {
                if (r + (uint64_t)u * step >= r_hi) break;
                const uint64_t key = qs_key(v[u]);
                const uint64_t pre = bits == 0u ? 0ull : key >> psh;
                for (uint32_t s = s_lo; s < s_hi; ++s)
                    if (pre == s_pv[s]) {
                        atomicAdd(&s_h[s * 256u + (uint32_t)((key >> dsh) & 255u)], 1u);
                        if (key == ~0ull) atomicAdd(&s_nan[s], 1u);
                        break;
                    }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < ns * 256u; i += QS_THREADS) {
        const uint32_t c = s_h[i];
        if (c) atomicAdd(&hist[(uint64_t)p0 * 256u + i], (unsigned long long)c);
    }
    if (threadIdx.x < ns && s_nan[threadIdx.x]) atomicAdd(&n_nan[p0 + threadIdx.x], (unsigned long long)s_nan[threadIdx.x]);
}

}  // inline namespace BPM_VARIANT_NS
}  // namespace bpm
