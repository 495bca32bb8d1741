// THE TAIL OF EVERY DATUM'S LOG DENSITIES: per datum i of the caller's data the K_i smallest finite l_is = ln_like_point(row s, datum i) over the
// rows s of a window of the resident history, exactly, and the log-sum-exp of -l over the rest -- what Pareto smoothed importance sampling needs
// (psis.h fits and finishes; bipymc_amd/pointwise.py: param_est_loo).  DEVICE CODE OF A RUN-TIME PROGRAM (hiprtc; pointwise.h:
// compile_pointwise_tail puts `#define BPM_POINTWISE_W w`, the caller's source and this file together), three kernels:
//
//   bpm_pointwise_tail        STAGE A, streaming.  Thread t of the workgroup of (data tile j, row part p) owns datum i = 256 (tile0 + j) + t and meets
//                             the part's rows in ascending order, staged as pointwise_rows.h stages them.  Its candidates live in a column of a
//                             slot-major buffer in global memory, buf[slot * 256 + t] (the lanes' appends and reads coalesce), of capacity 2 K_i,
//                             as order-preserving 64-bit keys.  A finite l is appended when its key is below the lane's threshold key (all bits set until the first compaction).
//                             After every row the workgroup asks whether ANY lane is full (__syncthreads_or); if so ALL lanes compact in lockstep:
//                             a lane with more than K_i candidates finds its K_i-th smallest key by an MSD radix select over its own column
//                             (4 bits a pass, its 16 counters in LDS at hist[digit * 256 + t]), keeps the keys below it and as many equal to it as
//                             make K_i, and sets thr to it.  A value equal to thr is not needed later: K_i values <= thr are already kept.
//                             What is not finite is counted and never kept.
//                             At its end a part compacts once more: it hands on at most K_i candidates.
//   bpm_pointwise_tail_final  A thread per datum, a workgroup per data tile: the parts' columns are concatenated into part 0's -- a lane appends
//                             what is below its threshold until its column is full or the part is through, without a barrier per value;
//                             the workgroup meets when no lane can go on, compacts, and continues -- one more compaction leaves min(K_i,
//                             finite values) keys, which go out datum-major,
//                             out[(256 j + t) * k_max + slot], padded to k_max with the largest key (the library's segmented sort then sorts
//                             columns of one length), with their number and the number of values that were not finite.
//   bpm_pointwise_body        STAGE B, on pointwise.h's fixed layout (parts and rows per part a function of (rows, n_data, d) alone): the online
//                             log-sum-exp (m, s) of pointwise_rows.h applied to x = -l over the rows with l >= cut_i, and their number; one record
//                             (part, datum) each, folded in part order by psis.h's kernel with pw_merge_lse.
// Selection is exact, so stage A's layout (parts, the data batch) may depend on the free memory; stage B's and psis.h's arithmetic may not and
// does not.  No atomics; a lane writes only its own column and its own counters.
//
// THE KEY of a finite double: its bits with the sign bit flipped (positive) or all bits flipped (negative) -- unsigned order = numeric order.
#pragma once

#ifndef BPM_POINTWISE_W
#error "pointwise_tail.h is compiled around a caller's ln_like_point (BPM_POINTWISE_W: doubles per datum)"
#endif
#define BPM_PT_HIST_WORDS 4096      // 16 counters x 256 lanes
#define BPM_PT_UNROLL 8u
#include "pointwise_datum.h"      // the opening of the pointwise kernels; through derive_rows.h the fixed-width typedefs, bpm_stage_rows

__device__ __forceinline__ unsigned long long bpm_pt_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double bpm_pt_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// One lane's candidates: col[slot * 256], slot < cnt; it keeps at most K (0: a lane without a datum, which never appends)
struct BpmPtLane {
    unsigned long long* col;
    unsigned int cnt, K;
    unsigned long long thr;      // a key: only keys below it are appended (all bits set: nothing was compacted yet)
};

// The K-th smallest key (1 <= K <= cnt) of the lane's column; *n_eq: how many keys equal to it belong to the K smallest.  hist: the lane's
// 16 counters at hist[digit * 256].
__device__ __forceinline__ unsigned long long bpm_pt_select(const BpmPtLane& a, unsigned int* hist, unsigned int* n_eq) {
    unsigned long long prefix = 0ull;
    unsigned int k = a.K;
    for (int shift = 60; shift >= 0; shift -= 4) {
        const unsigned long long above = shift == 60 ? 0ull : (~0ull << (shift + 4));
        for (unsigned int g = 0; g < 16u; ++g) hist[g * 256u] = 0u;
        for (unsigned int j0 = 0; j0 < a.cnt; j0 += BPM_PT_UNROLL) {      // BPM_PT_UNROLL loads in flight: the column is read at the latency of global memory
            unsigned long long key[BPM_PT_UNROLL];
#pragma unroll
            for (unsigned int u = 0; u < BPM_PT_UNROLL; ++u) key[u] = a.col[(unsigned long long)(j0 + u < a.cnt ? j0 + u : a.cnt - 1u) * 256ull];
#pragma unroll
            for (unsigned int u = 0; u < BPM_PT_UNROLL; ++u)
                if (j0 + u < a.cnt && (key[u] & above) == prefix) hist[(unsigned int)((key[u] >> shift) & 15ull) * 256u] += 1u;
        }
        unsigned int g = 0u;
        for (; g < 15u; ++g) {
            const unsigned int c = hist[g * 256u];
            if (c >= k) break;
            k -= c;
        }
        prefix |= (unsigned long long)g << shift;
    }
    *n_eq = k;
    return prefix;
}

// The lane keeps its K smallest (nothing to do with K or fewer candidates): in place, the kept keys in their order of arrival
__device__ __forceinline__ void bpm_pt_compact(BpmPtLane& a, unsigned int* hist) {
    if (a.K == 0u || a.cnt <= a.K) return;
    unsigned int n_eq = 0u;
    const unsigned long long kth = bpm_pt_select(a, hist, &n_eq);
    unsigned int w = 0u;
    for (unsigned int j0 = 0; j0 < a.cnt; j0 += BPM_PT_UNROLL) {
        unsigned long long key[BPM_PT_UNROLL];
#pragma unroll
        for (unsigned int u = 0; u < BPM_PT_UNROLL; ++u) key[u] = a.col[(unsigned long long)(j0 + u < a.cnt ? j0 + u : a.cnt - 1u) * 256ull];
#pragma unroll
        for (unsigned int u = 0; u < BPM_PT_UNROLL; ++u) {
            if (j0 + u >= a.cnt) break;
            bool keep = key[u] < kth;
            if (key[u] == kth && n_eq > 0u) { keep = true; --n_eq; }
            if (keep) { a.col[(unsigned long long)w * 256ull] = key[u]; ++w; }      // (w <= j0 + u, and the batch was read before any of its slots is written)
        }
    }
    a.cnt = w;
    a.thr = kth;
}

// One step of every lane of the workgroup (all 256 threads call it): append `l` where `take` and its key is below thr; then, if any lane is full, all compact.
// -> whether the workgroup compacted.  Before the call every lane has cnt < 2 K (or K = 0); after it too.
__device__ __forceinline__ bool bpm_pt_push(BpmPtLane& a, bool take, double l, unsigned int* hist) {
    const unsigned long long key = bpm_pt_key(l);
    if (take && a.K != 0u && key < a.thr) {      // (compared as keys, the order the select uses: -0.0 is below +0.0)
        a.col[(unsigned long long)a.cnt * 256ull] = key;
        ++a.cnt;
    }
    const int full = a.K != 0u && a.cnt >= 2u * a.K;
    if (!__syncthreads_or(full)) return false;
    bpm_pt_compact(a, hist);
    return true;
}

__device__ __forceinline__ bool bpm_pt_finite(double l) { return l - l == 0.0; }      // (inf - inf and NaN - NaN are NaN)

extern "C" __global__ void __launch_bounds__(256) bpm_pointwise_tail(const double* H, unsigned int ld, int d, unsigned long long lo, unsigned long long hi,
                                                                     unsigned long long chunk, unsigned int n_tiles, unsigned int tile0, const double* params,
                                                                     const double* data, unsigned int n_data, unsigned int R, unsigned int ldp,
                                                                     unsigned int lds_rows, const unsigned int* keep, unsigned int cap,
                                                                     unsigned long long* buf, unsigned int* cnt_out, unsigned int* bad_out,
                                                                     unsigned int* compactions) {
    extern __shared__ __attribute__((aligned(16))) double bpm_lds[];
    unsigned int* const hist = reinterpret_cast<unsigned int*>(bpm_lds + lds_rows) + threadIdx.x;
    BPM_PW_OPEN(tile0)
    BpmPtLane a;
    a.col = buf + (unsigned long long)blockIdx.x * cap * 256ull + tid;
    a.cnt = 0u;
    a.K = live ? keep[i] : 0u;
    a.thr = ~0ull;
    unsigned int n_bad = 0u, n_compact = 0u;
    for (unsigned long long t0 = r0; t0 < r1; t0 += R) {
        const unsigned int nr = bpm_pw_stage_tile(bpm_lds, H, ld, d, t0, r1, R, ldp);
        for (unsigned int r = 0; r < nr; ++r) {      // (every thread, live or not: the step below holds a barrier)
            double l = 0.0;
            bool fin = false;
            if (live) {
                const double* x = ldp != 0u ? bpm_lds + r * ldp : H + (t0 + r) * ld;
                l = ln_like_point(x, d, y, (int)i, params);
                fin = bpm_pt_finite(l);
                if (!fin) ++n_bad;
            }
            if (bpm_pt_push(a, fin, l, hist)) ++n_compact;
        }
    }
    bpm_pt_compact(a, hist);      // (not counted: the part hands on at most K candidates)
    const unsigned long long q = (unsigned long long)blockIdx.x * 256ull + tid;
    cnt_out[q] = a.cnt;
    bad_out[q] = n_bad;
    if (tid == 0u) compactions[blockIdx.x] = n_compact;
}

// buf, cnt, bad: what bpm_pointwise_tail left, workgroup (tile j, part p) at index p * n_tiles + j.  out: n_tiles * 256 columns of k_max keys.
extern "C" __global__ void __launch_bounds__(256) bpm_pointwise_tail_final(unsigned int n_tiles, unsigned int tile0, unsigned int parts, unsigned int n_data,
                                                                           const unsigned int* keep, unsigned int cap, unsigned int k_max,
                                                                           unsigned long long* buf, const unsigned int* cnt, const unsigned int* bad,
                                                                           unsigned long long* out, unsigned int* n_kept, unsigned int* n_bad) {
    __shared__ unsigned int hist_all[BPM_PT_HIST_WORDS];
    const unsigned int tid = threadIdx.x, tile = blockIdx.x;
    unsigned int* const hist = hist_all + tid;
    const unsigned long long i = ((unsigned long long)tile0 + tile) * 256ull + tid;
    const bool live = i < n_data;
    BpmPtLane a;
    a.col = buf + (unsigned long long)tile * cap * 256ull + tid;
    a.cnt = cnt[(unsigned long long)tile * 256ull + tid];
    a.K = live ? keep[i] : 0u;
    a.thr = ~0ull;
    unsigned int nb = bad[(unsigned long long)tile * 256ull + tid];
    bpm_pt_compact(a, hist);      // (at most K kept: room for K more)
    for (unsigned int p = 1; p < parts; ++p) {
        const unsigned long long wg = (unsigned long long)p * n_tiles + tile;
        const unsigned long long* src = buf + wg * cap * 256ull + tid;
        const unsigned int n = cnt[wg * 256ull + tid];
        nb += bad[wg * 256ull + tid];
        unsigned int j = 0u;
        for (;;) {      // the lane appends what is below its threshold until its column is full or the part is through; no barrier per value
            while (j < n && a.cnt < 2u * a.K) {
                const unsigned long long key = src[(unsigned long long)j * 256ull];
                ++j;
                if (key < a.thr) { a.col[(unsigned long long)a.cnt * 256ull] = key; ++a.cnt; }
            }
            if (!__syncthreads_or(j < n)) break;      // (every lane is through this part)
            bpm_pt_compact(a, hist);                  // a lane that stopped is full: K of its 2 K go
        }
    }
    bpm_pt_compact(a, hist);
    unsigned long long* o = out + ((unsigned long long)tile * 256ull + tid) * k_max;
    for (unsigned int j = 0; j < k_max; ++j) o[j] = j < a.cnt ? a.col[(unsigned long long)j * 256ull] : ~0ull;
    n_kept[(unsigned long long)tile * 256ull + tid] = a.cnt;
    n_bad[(unsigned long long)tile * 256ull + tid] = nb;
}

// rec: three fields of n_rec = parts * n_cols records, field f of (part p, column q = 256 tile + t) at rec[f * n_rec + p * n_cols + q]:
// the number of rows with l >= cut (a 64-bit word), and (m, s) of x = -l over them.  cut[q]: NaN where the datum has no cutoff (no row counts).
extern "C" __global__ void __launch_bounds__(256) bpm_pointwise_body(const double* H, unsigned int ld, int d, unsigned long long lo, unsigned long long hi,
                                                                     unsigned long long chunk, unsigned int n_tiles, unsigned int tile0, const double* params,
                                                                     const double* data, unsigned int n_data, unsigned int R, unsigned int ldp,
                                                                     const double* cut, double* rec, unsigned long long n_rec) {
    extern __shared__ __attribute__((aligned(16))) double bpm_lds[];
    BPM_PW_OPEN(tile0)
    const unsigned long long q = (unsigned long long)tile * 256ull + tid, n_cols = (unsigned long long)n_tiles * 256ull;
    const double c = cut[q];
    unsigned long long n = 0ull;
    double m = 0.0, s = 0.0;
    for (unsigned long long t0 = r0; t0 < r1; t0 += R) {
        const unsigned int nr = bpm_pw_stage_tile(bpm_lds, H, ld, d, t0, r1, R, ldp);
        if (!live) continue;
        for (unsigned int r = 0; r < nr; ++r) {
            const double* x = ldp != 0u ? bpm_lds + r * ldp : H + (t0 + r) * ld;
            const double l = ln_like_point(x, d, y, (int)i, params);
            if (!(bpm_pt_finite(l) && l >= c)) continue;
            const double v = -l;
            const bool first = n == 0ull;
            const BpmPwLse ms = bpm_pw_lse_add(first, m, s, v);
            m = ms.m; s = ms.s;
            ++n;
        }
    }
    const unsigned long long j = (unsigned long long)part * n_cols + q;
    reinterpret_cast<unsigned long long*>(rec)[j] = n;
    rec[n_rec + j] = m;
    rec[2ull * n_rec + j] = s;
}
