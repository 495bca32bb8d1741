// Per-generation trace summaries of the resident history: what the reference's trace plots draw from the gathered chains
// (plot_mcmc_indep_chains / plot_mcmc_chain, mc_plot/mc_plot.py:52-102: one line per chain, np.mean and np.std per generation), reduced
// where the history lives.  The host (bipymc_amd/traces.py) merges the ranks and finishes mean and sd.
//
// A generation g is a contiguous block: n_local rows of ld doubles at H[(g * n_local + i) * ld + k], n_local doubles at LL[g * n_local + i].
// Bin t pools the generations [g_lo + t * every, min(g_lo + (t + 1) * every, g_hi)), so a bin is a contiguous range of local rows; a bin
// is cut into gridDim.y contiguous parts of ceil(rows / parts) rows (the last ones may be empty), one workgroup each.
//
// What is accumulated per (bin, coordinate), the same for the ln-like column: over the finite values their count n, a shift c and the
// shifted sums S1 = sum (x - c), S2 = sum (x - c)^2; how many values are NaN; min and max over the values that are not NaN (the
// infinities among them: they show there and nowhere else).  c is the first finite value the accumulator met, a value of the bin itself,
// so a history far from the origin does not cancel: S2 / n <= var + (c - mean)^2 <= 2 max |x - mean|^2.  Two accumulators A, B merge into
// A's shift with d = c_B - c_A:  S1 = S1_A + (S1_B + n_B d),  S2 = S2_A + (S2_B + (2 d S1_B + n_B d^2))  (tr_merge_moments), min / max / counts
// the obvious way.  Every merge runs in a fixed order -- a lane's rows ascending, the lanes of a coordinate by a halving tree in LDS, the
// parts of a bin in index order (tr_fold_kernel) -- and there is no atomic, so the bits do not depend on how the workgroups were scheduled.
// The first accumulator in that order starts at the bin's first row: c is the rank's first row of the bin wherever that value is finite.
//
//   tr_bins_kernel    grid (column tiles x bins, parts), the tile index fastest (workgroups that read the same rows run side by side).  The
//                     lane layout of hs_range_kernel (histograms.h): lane = a * kw + kk reads coordinate tile * kw + kk of the rows lo + a,
//                     step cpw = TR_THREADS / kw, TR_UNR independent loads in flight; one pass, every element read once for all results.
//                     Rows wider than TR_THREADS coordinates are more column tiles.
//   tr_ll_kernel      grid (bins, parts): the same over the one ln-like column, 256 consecutive entries per load.  Also counts +inf and
//                     -inf apart and finds the arg-max: the largest order-preserving key (qs_key of x + 0.0: -0.0 counts as 0.0) of the values
//                     that are not NaN with the smallest local row that carries it, compared as integers.
//   tr_fold_kernel    one lane per (bin, coordinate): the parts of a bin in index order.
//   tr_gather_kernel  one lane per (bin, requested chain, coordinate or ln-like): the chain's row at the bin's first generation, dense.
// Records are structure-of-arrays: field f of record j at rec[f * n_rec + j]; part records j = (t * parts + p) * ld + k, folded records
// j = t * ld + k (ld = 1 for the ln-likes) -- with one part the part records are the folded ones.  Counts leave as 64-bit words.
#pragma once
#include "kernels.h"
#include "quantiles.h"
#include "trace_acc.h"      // TrAcc, tr_init / tr_add / tr_merge_moments / tr_merge / tr_store, the field enum (shared with derived.h)

namespace bpm {
inline namespace BPM_VARIANT_NS {      // (philox.h: one kernel-symbol namespace per build variant)

constexpr int TR_THREADS = 256;
constexpr int TR_UNR = 4;                      // independent loads in flight per lane
constexpr uint64_t TR_NO_ROW = ~0ull;          // arg-max: no value that is not NaN (its key is 0, below every key)

struct TrLlAcc {
    TrAcc m;
    uint32_t n_pinf, n_ninf;
    uint64_t bkey, brow;
};

// the larger key wins, the smaller row among equal keys
__device__ __forceinline__ void tr_merge_best(uint64_t& key, uint64_t& row, uint64_t kb, uint64_t rb) {
    if (kb > key || (kb == key && rb < row)) { key = kb; row = rb; }
}

// this workgroup's rows [lo, hi) of bin t
__device__ __forceinline__ void tr_part(uint64_t t, uint32_t n_local, uint64_t g_lo, uint64_t g_hi, uint64_t every, uint64_t* lo, uint64_t* hi) {
    const uint64_t ga = g_lo + t * every, gb = ga + every < g_hi ? ga + every : g_hi;
    const uint64_t r0 = ga * n_local, r1 = gb * n_local, chunk = (r1 - r0 + gridDim.y - 1) / gridDim.y;
    const uint64_t a = r0 + (uint64_t)blockIdx.y * chunk;
    *lo = a < r1 ? a : r1;
    *hi = *lo + chunk < r1 ? *lo + chunk : r1;
}

// rec: TR_F_BINS fields of n_rec = bins * parts * ld part records
__global__ __launch_bounds__(TR_THREADS) void tr_bins_kernel(const double* __restrict__ H, uint32_t ld, uint32_t n_local, uint64_t g_lo, uint64_t g_hi,
                                                             uint64_t every, uint32_t kw, uint32_t n_tiles, double* __restrict__ rec, uint64_t n_rec) {
    __shared__ TrAcc s_acc[TR_THREADS];
    const uint32_t tile = blockIdx.x % n_tiles;
    const uint64_t t = blockIdx.x / n_tiles;
    const uint32_t cpw = TR_THREADS / kw, a = threadIdx.x / kw, kk = threadIdx.x % kw;
    const uint32_t k = tile * kw + kk;
    uint64_t lo, hi;
    tr_part(t, n_local, g_lo, g_hi, every, &lo, &hi);
    TrAcc acc;
    tr_init(acc);
    if (a < cpw && k < ld) {
        for (uint64_t r = lo + a; r < hi; r += (uint64_t)cpw * TR_UNR) {
            double v[TR_UNR];
#pragma unroll
            for (int u = 0; u < TR_UNR; ++u) {
                const uint64_t rr = r + (uint64_t)u * cpw;
                v[u] = 0.0;
                if (rr < hi) v[u] = H[rr * ld + k];
            }
#pragma unroll
            for (int u = 0; u < TR_UNR; ++u) {
                if (r + (uint64_t)u * cpw >= hi) break;
                tr_add(acc, v[u]);
            }
        }
    }
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    uint32_t top = 1u;
    while (top < cpw) top <<= 1;
    for (uint32_t s = top >> 1; s > 0u; s >>= 1) {      // the cpw lanes of a coordinate: a halving tree, the same pairs every time
        if (a < s && a + s < cpw) tr_merge(s_acc[threadIdx.x], s_acc[threadIdx.x + s * kw]);
        __syncthreads();
    }
    if (a == 0u && k < ld) tr_store(rec, n_rec, (t * gridDim.y + blockIdx.y) * ld + k, s_acc[threadIdx.x]);
}

// rec: TR_F_LL fields of n_rec = bins * parts part records
__global__ __launch_bounds__(TR_THREADS) void tr_ll_kernel(const double* __restrict__ LL, uint32_t n_local, uint64_t g_lo, uint64_t g_hi, uint64_t every,
                                                           double* __restrict__ rec, uint64_t n_rec) {
    __shared__ TrLlAcc s_acc[TR_THREADS];
    const uint64_t t = blockIdx.x;
    uint64_t lo, hi;
    tr_part(t, n_local, g_lo, g_hi, every, &lo, &hi);
    TrLlAcc acc;
    tr_init(acc.m);
    acc.n_pinf = acc.n_ninf = 0u;
    acc.bkey = 0ull;
    acc.brow = TR_NO_ROW;
    for (uint64_t r = lo + threadIdx.x; r < hi; r += (uint64_t)TR_THREADS * TR_UNR) {
        double v[TR_UNR];
#pragma unroll
        for (int u = 0; u < TR_UNR; ++u) {
            const uint64_t rr = r + (uint64_t)u * TR_THREADS;
            v[u] = 0.0;
            if (rr < hi) v[u] = LL[rr];
        }
#pragma unroll
        for (int u = 0; u < TR_UNR; ++u) {
            const uint64_t rr = r + (uint64_t)u * TR_THREADS;
            if (rr >= hi) break;
            const double x = v[u];
            if (!tr_add(acc.m, x) && x == x) {
                if (x > 0.0) ++acc.n_pinf;
                else ++acc.n_ninf;
            }
            if (x == x) {
                const uint64_t key = qs_key(x + 0.0);
                if (key > acc.bkey) { acc.bkey = key; acc.brow = rr; }      // (rows ascend: the first of equal keys stays)
            }
        }
    }
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t s = TR_THREADS / 2; s > 0u; s >>= 1) {
        if (threadIdx.x < s) {
            TrLlAcc& x = s_acc[threadIdx.x];
            const TrLlAcc& y = s_acc[threadIdx.x + s];
            tr_merge(x.m, y.m);
            x.n_pinf += y.n_pinf;
            x.n_ninf += y.n_ninf;
            tr_merge_best(x.bkey, x.brow, y.bkey, y.brow);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0u) {
        const uint64_t j = t * gridDim.y + blockIdx.y;
        unsigned long long* u = reinterpret_cast<unsigned long long*>(rec);
        tr_store(rec, n_rec, j, s_acc[0].m);
        u[TR_PINF * n_rec + j] = s_acc[0].n_pinf;
        u[TR_NINF * n_rec + j] = s_acc[0].n_ninf;
        u[TR_BKEY * n_rec + j] = s_acc[0].bkey;
        u[TR_BROW * n_rec + j] = s_acc[0].brow;
    }
}

// part: n_fields fields of n_out * parts part records; out: n_fields fields of n_out folded records (n_out = bins * ld)
__global__ __launch_bounds__(TR_THREADS) void tr_fold_kernel(const double* __restrict__ part, uint32_t parts, uint32_t ld, uint64_t n_out, uint32_t n_fields,
                                                             double* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * TR_THREADS + threadIdx.x;
    if (j >= n_out) return;
    const uint64_t t = j / ld, k = j % ld, n_rec = n_out * parts;
    const unsigned long long* pu = reinterpret_cast<const unsigned long long*>(part);
    unsigned long long* ou = reinterpret_cast<unsigned long long*>(out);
    unsigned long long n = 0ull, n_nan = 0ull, n_pinf = 0ull, n_ninf = 0ull, bkey = 0ull, brow = TR_NO_ROW;
    double c = 0.0, s1 = 0.0, s2 = 0.0, mn = __longlong_as_double(0x7FF0000000000000ll), mx = -mn;
    for (uint32_t p = 0; p < parts; ++p) {
        const uint64_t q = (t * parts + p) * ld + k;
        tr_merge_moments(n, c, s1, s2, pu[TR_N * n_rec + q], part[TR_C * n_rec + q], part[TR_S1 * n_rec + q], part[TR_S2 * n_rec + q]);
        n_nan += pu[TR_NAN * n_rec + q];
        const double a = part[TR_MIN * n_rec + q], b = part[TR_MAX * n_rec + q];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        if (n_fields == (uint32_t)TR_F_LL) {
            n_pinf += pu[TR_PINF * n_rec + q];
            n_ninf += pu[TR_NINF * n_rec + q];
            uint64_t bk = bkey, br = brow;
            tr_merge_best(bk, br, pu[TR_BKEY * n_rec + q], pu[TR_BROW * n_rec + q]);
            bkey = bk; brow = br;
        }
    }
    ou[TR_N * n_out + j] = n;
    out[TR_C * n_out + j] = c;
    out[TR_S1 * n_out + j] = s1;
    out[TR_S2 * n_out + j] = s2;
    ou[TR_NAN * n_out + j] = n_nan;
    out[TR_MIN * n_out + j] = mn;
    out[TR_MAX * n_out + j] = mx;
    if (n_fields == (uint32_t)TR_F_LL) {
        ou[TR_PINF * n_out + j] = n_pinf;
        ou[TR_NINF * n_out + j] = n_ninf;
        ou[TR_BKEY * n_out + j] = bkey;
        ou[TR_BROW * n_out + j] = brow;
    }
}

// ids: n_ids local chains; out_x[(t * n_ids + j) * dim + k], out_ll[t * n_ids + j]: chain ids[j] at generation g_lo + t * every, t < bins
__global__ __launch_bounds__(TR_THREADS) void tr_gather_kernel(const double* __restrict__ H, const double* __restrict__ LL, uint32_t ld, uint32_t dim,
                                                               uint32_t n_local, uint64_t g_lo, uint64_t every, uint64_t bins, uint32_t n_ids,
                                                               const uint32_t* __restrict__ ids, double* __restrict__ out_x, double* __restrict__ out_ll) {
    const uint64_t i = (uint64_t)blockIdx.x * TR_THREADS + threadIdx.x;
    if (i >= bins * n_ids * (dim + 1u)) return;
    const uint32_t kk = (uint32_t)(i % (dim + 1u));
    const uint64_t tj = i / (dim + 1u), t = tj / n_ids;
    const uint64_t r = (g_lo + t * every) * n_local + ids[tj % n_ids];
    if (kk < dim) out_x[tj * dim + kk] = H[r * ld + kk];
    else out_ll[tj] = LL[r];
}

}  // inline namespace BPM_VARIANT_NS
}  // namespace bpm
