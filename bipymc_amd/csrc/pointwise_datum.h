// THE COMMON OPENING OF THE POINTWISE KERNELS: what bpm_pointwise_rows (pointwise_rows.h), bpm_pointwise_tail and bpm_pointwise_body
// (pointwise_tail.h) share.  DEVICE CODE OF A RUN-TIME PROGRAM (hiprtc), included after `#define BPM_POINTWISE_W w` and the caller's source.
//   BPM_PW_OPEN(tile0)   the workgroup of (data tile, row part) = (blockIdx.x % n_tiles, blockIdx.x / n_tiles): thread `tid` owns datum
//                        i = 256 (tile0 + tile) + tid, `live` if there is one; the part's rows are [r0, r1), `chunk` of the window [lo, hi); `y`:
//                        the datum's w values -- in registers (yv[]) when w <= BPM_PW_W_REGS, else where they lie.  A MACRO, not a function: it
//                        declares the kernel's own locals from its parameters (n_tiles, n_data, lo, hi, chunk, data), and yv[] handed back by a
//                        function would be an array behind a pointer -- it must stay in VGPRs, never scratch (profiles/waic_cfg2.txt).
//   bpm_pw_stage_tile    one tile of the part's rows, [t0, t0 + nr), staged into LDS as derive_rows.h stages rows (ldp == 0: left where it lies).
//   bpm_pw_lse_add       one step of the online log-sum-exp (m, s) (pointwise_rows.h, THE ORDER OF OPERATIONS, step 2).
#pragma once
#if BPM_POINTWISE_W < 1 || BPM_POINTWISE_W > 64
#error "BPM_POINTWISE_W (doubles per datum) must be 1 ... 64"
#endif
#define BPM_PW_W_REGS 8
#define BPM_STAGE_ROWS_ONLY
#include "derive_rows.h"      // the fixed-width typedefs, trace_acc.h, bpm_stage_rows

#if BPM_POINTWISE_W <= BPM_PW_W_REGS
#define BPM_PW_Y                                                                                                              \
    double yv[BPM_POINTWISE_W];                                                                                               \
    _Pragma("unroll") for (int k = 0; k < BPM_POINTWISE_W; ++k) yv[k] = live ? data[i * BPM_POINTWISE_W + k] : 0.0;           \
    const double* y = yv;
#else
#define BPM_PW_Y const double* y = data + (live ? i : 0ull) * BPM_POINTWISE_W;
#endif
#define BPM_PW_OPEN(tile0)                                                                                                    \
    const unsigned int tid = threadIdx.x, tile = blockIdx.x % n_tiles, part = blockIdx.x / n_tiles;                          \
    const unsigned long long i = ((unsigned long long)(tile0) + tile) * 256ull + tid;                                        \
    const bool live = i < n_data;                                                                                             \
    unsigned long long r0 = lo + (unsigned long long)part * chunk;                                                            \
    r0 = r0 < hi ? r0 : hi;                                                                                                   \
    const unsigned long long r1 = r0 + chunk < hi ? r0 + chunk : hi;                                                          \
    BPM_PW_Y

// every thread of the workgroup calls it (it holds barriers) -> nr, the rows of the tile: min(R, r1 - t0)
__device__ __forceinline__ unsigned int bpm_pw_stage_tile(double* lds, const double* H, unsigned int ld, int d, unsigned long long t0, unsigned long long r1,
                                                          unsigned int R, unsigned int ldp) {
    const unsigned int nr = (unsigned int)(r1 - t0 < R ? r1 - t0 : R);
    if (ldp != 0u) {
        __syncthreads();      // (the previous tile has been read by every thread)
        bpm_stage_rows(lds, H, ld, d, t0, nr, ldp);
        __syncthreads();
    }
    return nr;
}

// (m, s) after it took in the finite value v -- first: it is the first one.  Every exp has a finite argument <= 0.  By value, not through
// references, and called with named arguments: that form compiles to the code the step had when each kernel spelled it out.
struct BpmPwLse { double m, s; };
__device__ __forceinline__ BpmPwLse bpm_pw_lse_add(bool first, double m, double s, double v) {
    if (first) return {v, 1.0};
    if (v > m) return {v, s * exp(m - v) + 1.0};
    return {m, s + exp(v - m)};
}
