// Posterior covariance of the resident history (the reference's only view of how the parameters move together is corner.corner over the
// gathered super chain, mc_plot/mc_plot.py:16-29): the centred sums S1[k] = sum (x_k - c_k) and S2[i][j] = sum (x_i - c_i)(x_j - c_j) over
// a window of local super-chain rows, a tall-skinny FP64 SYRK on the matrix cores.  bipymc_amd/covariance.py chooses the centre (the global
// mean), merges the ranks and finishes cov / corr.
//
// The window is a contiguous range [r_lo, r_hi) of local super-chain rows; row r holds its coordinates at H[r * ld + k], k < ld.  Columns
// are cut into tiles of 16.  v_mfma_f64_16x16x4_f64 computes D[i][j] += sum_{k < 4} A[i][k] B[k][j] with lane l holding A[i = l & 15][k = l >> 4]
// and B[k = l >> 4][j = l & 15]: with k a row of the window and i, j columns of two tiles, the value y = H[(r0 + (l >> 4)) * ld + k0 + (l & 15)]
// - c[k0 + (l & 15)] is at once the A operand of tile k0 and the B operand of tile k0, so a tile of 4 rows is loaded once (16 consecutive
// doubles of each row) and used against every other tile.  Result map of the f64 form: lane l, register q holds D[row (l >> 4) + 4 q][col l & 15].
// Columns >= dim and rows >= r_hi are set to 0 after the subtraction.
//
//   cov_partial_kernel<T, DIAG>   one wavefront per workgroup, grid (nbx, blocks).  Column tiles are cut into blocks of T tiles (one block of
//                                 T <= COV_MAX_T tiles where that covers dim, blocks of COV_BLK otherwise).  DIAG: block bi against itself,
//                                 the T (T + 1) / 2 tile pairs ta <= tb, and S1 of its columns (the operand registers added per lane).
//                                 Otherwise block pair bi < bj (blockIdx.y counts them row by row), T x T tile pairs.  Workgroup bx walks the
//                                 groups of 4 rows bx, bx + nbx, ..., COV_UNR groups per step, the next step's loads in flight while this step
//                                 multiplies.  Accumulators (8 registers per tile pair) go to part[slot][bx][pair][q][lane], slot = bi for
//                                 DIAG, n_blk + pair index otherwise; S1 to part1[bi][bx][t][lane].
//   cov_final_kernel              adds the nbx partials of one tile pair in a fixed order (4 contiguous slices, each in order, then the 4
//                                 slice sums in order) and writes the upper-triangle elements and their mirror images into cross[dim][dim].
//   cov_sum_final_kernel          the same for S1 (the 4 row lanes of a column inside each slice, in order).
// No floating-point atomics anywhere: the same rows give the same bits.
#pragma once
#include "kernels.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {      // (philox.h: one kernel-symbol namespace per build variant)

constexpr int COV_MAX_T = 7;       // tiles of the single-block form: dim <= 112, 28 tile pairs = 224 accumulator registers per lane
constexpr int COV_BLK = 4;         // tiles per block beyond that: 16 (10 on the diagonal) tile pairs = 128 accumulator registers
constexpr int COV_UNR = 4;         // groups of 4 rows per step
constexpr int COV_FIN_THREADS = 1024;
typedef double cov_acc_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void cov_block_pair(uint32_t p, uint32_t n_blk, uint32_t& bi, uint32_t& bj) {
    bi = 0;
    while (p >= n_blk - 1u - bi) { p -= n_blk - 1u - bi; ++bi; }
    bj = bi + 1u + p;
}

template <int T, bool DIAG>
__global__ __launch_bounds__(64) void cov_partial_kernel(const double* __restrict__ H, uint32_t ld, uint32_t dim, uint64_t r_lo, uint64_t r_hi,
                                                         const double* __restrict__ center, uint32_t n_blk, double* __restrict__ part,
                                                         double* __restrict__ part1) {
    constexpr int TB = DIAG ? 1 : T;     // operand tiles of the second block (DIAG: the first block's own)
    const uint32_t lane = threadIdx.x, lc = lane & 15u, lr = lane >> 4;
    uint32_t bi, bj;
    if (DIAG) bi = bj = blockIdx.y;
    else cov_block_pair(blockIdx.y, n_blk, bi, bj);
    const uint32_t slot = DIAG ? bi : n_blk + blockIdx.y;
    // this lane's column of every tile, clamped for the load; its centre; whether it is a column of the matrix
    uint32_t ka[T], kb[TB];
    double ca[T], cb[TB];
    bool oka[T], okb[TB];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint32_t k = (bi * T + t) * 16u + lc;
        oka[t] = k < dim;
        ka[t] = oka[t] ? k : dim - 1u;
        ca[t] = center[ka[t]];
    }
#pragma unroll
    for (int t = 0; t < TB; ++t) {
        const uint32_t k = (bj * T + t) * 16u + lc;
        okb[t] = k < dim;
        kb[t] = okb[t] ? k : dim - 1u;
        cb[t] = center[kb[t]];
    }
    cov_acc_t acc[T][T];
    double s1[T];
#pragma unroll
    for (int a = 0; a < T; ++a) {
        s1[a] = 0.0;
#pragma unroll
        for (int b = 0; b < T; ++b) acc[a][b] = cov_acc_t{0.0, 0.0, 0.0, 0.0};
    }
    const uint64_t n_grp = (r_hi - r_lo + 3u) / 4u;
    const uint64_t step = gridDim.x;
    double xa[COV_UNR][T], xb[COV_UNR][TB], na[COV_UNR][T], nb[COV_UNR][TB];
    bool okr[COV_UNR], nkr[COV_UNR];
    // loads of the COV_UNR groups g, g + step, ...: rows beyond the window read its last row (and are zeroed by okr)
    auto load = [&](uint64_t g, double (&va)[COV_UNR][T], double (&vb)[COV_UNR][TB], bool (&vk)[COV_UNR]) {
#pragma unroll
        for (int u = 0; u < COV_UNR; ++u) {
            const uint64_t r = r_lo + 4u * (g + (uint64_t)u * step) + lr;
            vk[u] = r < r_hi;
            const double* row = H + (vk[u] ? r : r_hi - 1u) * ld;
#pragma unroll
            for (int t = 0; t < T; ++t) va[u][t] = row[ka[t]];
            if (!DIAG) {
#pragma unroll
                for (int t = 0; t < TB; ++t) vb[u][t] = row[kb[t]];
            }
        }
    };
    uint64_t g = blockIdx.x;
    if (g < n_grp) load(g, xa, xb, okr);
    while (g < n_grp) {
        const uint64_t g_next = g + step * COV_UNR;
        if (g_next < n_grp) load(g_next, na, nb, nkr);
#pragma unroll
        for (int u = 0; u < COV_UNR; ++u) {
            double ya[T], yb[TB];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const double y = xa[u][t] - ca[t];
                ya[t] = (okr[u] && oka[t]) ? y : 0.0;
                if (DIAG) s1[t] += ya[t];
            }
            if (!DIAG) {
#pragma unroll
                for (int t = 0; t < TB; ++t) {
                    const double y = xb[u][t] - cb[t];
                    yb[t] = (okr[u] && okb[t]) ? y : 0.0;
                }
            }
#pragma unroll
            for (int a = 0; a < T; ++a) {
#pragma unroll
                for (int b = DIAG ? a : 0; b < T; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[a], DIAG ? ya[b] : yb[DIAG ? 0 : b], acc[a][b], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < COV_UNR; ++u) {
            okr[u] = nkr[u];
#pragma unroll
            for (int t = 0; t < T; ++t) xa[u][t] = na[u][t];
            if (!DIAG) {
#pragma unroll
                for (int t = 0; t < TB; ++t) xb[u][t] = nb[u][t];
            }
        }
        g = g_next;
    }
    double* out = part + ((uint64_t)slot * gridDim.x + blockIdx.x) * (uint64_t)(T * T * 256);
#pragma unroll
    for (int a = 0; a < T; ++a) {
#pragma unroll
        for (int b = DIAG ? a : 0; b < T; ++b) {
#pragma unroll
            for (int q = 0; q < 4; ++q) out[(a * T + b) * 256 + q * 64 + lane] = acc[a][b][q];
        }
    }
    if (DIAG) {
        double* o1 = part1 + ((uint64_t)bi * gridDim.x + blockIdx.x) * (uint64_t)(T * 64);
#pragma unroll
        for (int t = 0; t < T; ++t) o1[t * 64 + lane] = s1[t];
    }
}

// grid (T * T, slots), COV_FIN_THREADS threads: element e = q * 64 + lane of tile pair (ta, tb) of the slot's block pair
__global__ __launch_bounds__(COV_FIN_THREADS) void cov_final_kernel(const double* __restrict__ part, uint32_t nbx, uint32_t T, uint32_t n_blk,
                                                                    uint32_t dim, double* __restrict__ cross) {
    __shared__ double s_p[COV_FIN_THREADS];
    const uint32_t slot = blockIdx.y, ta = blockIdx.x / T, tb = blockIdx.x % T;
    uint32_t bi, bj;
    if (slot < n_blk) {
        bi = bj = slot;
        if (ta > tb) return;
    } else {
        cov_block_pair(slot - n_blk, n_blk, bi, bj);
    }
    const uint32_t ga = bi * T + ta, gb = bj * T + tb;
    if (ga * 16u >= dim || gb * 16u >= dim) return;
    const uint32_t e = threadIdx.x & 255u, sl = threadIdx.x >> 8;
    const uint32_t chunk = (nbx + 3u) / 4u;
    const uint32_t b_lo = sl * chunk < nbx ? sl * chunk : nbx, b_hi = b_lo + chunk < nbx ? b_lo + chunk : nbx;
    const double* p = part + ((uint64_t)slot * nbx * T * T + blockIdx.x) * 256u + e;
    const uint64_t stride = (uint64_t)T * T * 256u;
    double a = 0.0;
#pragma unroll 8
    for (uint32_t b = b_lo; b < b_hi; ++b) a += p[b * stride];
    s_p[threadIdx.x] = a;
    __syncthreads();
    if (sl == 0u) {
        const double v = ((s_p[e] + s_p[256u + e]) + s_p[512u + e]) + s_p[768u + e];
        const uint32_t lane = e & 63u, q = e >> 6;
        const uint32_t row = ga * 16u + (lane >> 4) + 4u * q, col = gb * 16u + (lane & 15u);
        if (row < dim && col < dim && row <= col) {
            cross[(uint64_t)row * dim + col] = v;
            cross[(uint64_t)col * dim + row] = v;
        }
    }
}

// grid (column tiles), 256 threads: column lc = thread & 15 of the tile; thread >> 4 = slice * 4 + row lane
__global__ __launch_bounds__(256) void cov_sum_final_kernel(const double* __restrict__ part1, uint32_t nbx, uint32_t T, uint32_t dim,
                                                            double* __restrict__ sum) {
    __shared__ double s_p[256];
    const uint32_t bi = blockIdx.x / T, t = blockIdx.x % T;
    const uint32_t lc = threadIdx.x & 15u, lr = (threadIdx.x >> 4) & 3u, sl = threadIdx.x >> 6;
    const uint32_t chunk = (nbx + 3u) / 4u;
    const uint32_t b_lo = sl * chunk < nbx ? sl * chunk : nbx, b_hi = b_lo + chunk < nbx ? b_lo + chunk : nbx;
    const double* p = part1 + ((uint64_t)bi * nbx * T + t) * 64u + lr * 16u + lc;
    const uint64_t stride = (uint64_t)T * 64u;
    double a = 0.0;
#pragma unroll 8
    for (uint32_t b = b_lo; b < b_hi; ++b) a += p[b * stride];
    s_p[threadIdx.x] = a;
    __syncthreads();
    const uint32_t k = blockIdx.x * 16u + lc;
    if (threadIdx.x < 16u && k < dim) {
        double v = 0.0;
        for (uint32_t j = 0; j < 16u; ++j) v += s_p[j * 16u + lc];
        sum[k] = v;
    }
}

}  // inline namespace BPM_VARIANT_NS
}  // namespace bpm
