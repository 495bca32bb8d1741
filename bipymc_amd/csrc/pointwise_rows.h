// THE POINTWISE LOG PREDICTIVE DENSITY: per datum i of the caller's data, the log-sum-exp and the moments of l_is = ln_like_point(row s, datum i)
// over the rows s of a window of the resident history -- what WAIC needs (pointwise.h has the host side; bipymc_amd/pointwise.py finishes).
// Two sections.  The first -- the record's fields and the merge of two log-sum-exps -- is plain C++ shared with the library (pointwise.h
// includes this file for it, BPM_POINTWISE_W undefined).  The second is DEVICE CODE OF A RUN-TIME PROGRAM (hiprtc; pointwise.h:
// compile_pointwise puts `#define BPM_POINTWISE_W w`, the caller's source and this file together): the kernel around the caller's
//     __device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p)      // y: the w values of datum i
//
// THE ORDER OF OPERATIONS -- a function of (n_rows, n_data, d) alone (pointwise.h: pointwise_layout; not of the device, the free memory or the
// environment), so that the result's bits are a function of (window, data, params) and of nothing else:
//   1. the window's rows [lo, hi) are cut into `parts` parts of `chunk` consecutive rows (the last one fewer); the data into tiles of T = 256;
//   2. thread t of the workgroup of (data tile j, part p) owns datum i = 256 j + t for the whole launch and meets the part's rows in ascending
//      order.  Per row, with l the caller's value:
//        l finite: the moments by trace_acc.h's tr_add (count n, shift c = the first finite l, S1 += l - c, S2 += (l - c)^2), and the online
//                  log-sum-exp (m, s):   the first finite l: m = l, s = 1;   l > m: s = s exp(m - l) + 1, m = l;   else s += exp(l - m)
//                  -- every exp has a finite argument <= 0: an infinite or NaN l never reaches it and m is never -inf where it is read,
//                  so no inf - inf is formed;
//        l = NaN, +inf, -inf: counted, each in its own counter, and nothing else;
//   3. the thread stores one record (part p, datum i), structure of arrays: field f at rec[f * n_rec + p * n_data + i], n_rec = parts * n_data;
//   4. the library's pw_fold_kernel, a thread per datum, merges the parts 0, 1, 2, ... in that order: the moments by tr_merge_moments, the
//      log-sum-exps by pw_merge_lse below; parts without a finite value are skipped.
// No atomics; the accumulators never leave registers.  A data tile with fewer than 256 data idles its spare lanes (they still help staging).
//
// The part's rows are staged R at a time into LDS by bpm_stage_rows (derive_rows.h: the staging of the derived quantities' kernels), row stride
// ldp = d | 1; every lane then reads the same x[j] of the same row -- an LDS broadcast, free of bank conflicts.  Rows too wide for a useful tile
// (ldp == 0) are read where they lie, at a wave-uniform address.  A datum's w values are read once into registers when w <= BPM_PW_W_REGS
// (no scratch: profiles/waic_cfg2.txt); above it the caller's function reads them where they lie, (n_data, w) row-major: consecutive lanes
// read consecutive data.  With `values` the thread stores l itself at values[(row - lo) * n_data + i]: consecutive lanes, consecutive addresses.
#pragma once

#if !defined(__HIPCC_RTC__) && !defined(__HIP_DEVICE_COMPILE__)
#include <math.h>
#endif
#if defined(__HIPCC__)
#define BPM_PW_HD __host__ __device__ __forceinline__      // (a plain C++ program states the same merge: tests/pointwise_host_main.cpp)
#else
#define BPM_PW_HD inline
#endif

// fields of a record (part or folded): counts are 64-bit words, the rest doubles
enum { PW_N = 0, PW_C, PW_S1, PW_S2, PW_NAN, PW_PINF, PW_NINF, PW_M, PW_S, PW_FIELDS };

// (m, s) of n_a finite values takes in (m_b, s_b) of n_b: the log-sum-exp of all is m + log(s), m the maximum.  An empty side is not read.
BPM_PW_HD void pw_merge_lse(unsigned long long n_a, double& m, double& s, unsigned long long n_b, double m_b, double s_b) {
    if (n_b == 0ull) return;
    if (n_a == 0ull) { m = m_b; s = s_b; return; }
    const double M = m_b > m ? m_b : m;
    s = s * exp(m - M) + s_b * exp(m_b - M);
    m = M;
}

#ifdef BPM_POINTWISE_W
#include "pointwise_datum.h"      // the opening of the pointwise kernels; through derive_rows.h the fixed-width typedefs, trace_acc.h, bpm_stage_rows

extern "C" __global__ void __launch_bounds__(256) bpm_pointwise_rows(const double* H, unsigned int ld, int d, unsigned long long lo, unsigned long long hi,
                                                                     unsigned long long chunk, unsigned int n_tiles, const double* params, const double* data,
                                                                     unsigned int n_data, unsigned int R, unsigned int ldp, double* rec,
                                                                     unsigned long long n_rec, double* values) {
    using namespace bpm;
    extern __shared__ __attribute__((aligned(16))) double bpm_lds[];
    BPM_PW_OPEN(0u)
    TrAcc acc;
    tr_init(acc);
    double m = acc.mx, s = 0.0;      // (-inf, 0: nothing yet)
    unsigned int n_pinf = 0u, n_ninf = 0u;
    for (unsigned long long t0 = r0; t0 < r1; t0 += R) {
        const unsigned int nr = bpm_pw_stage_tile(bpm_lds, H, ld, d, t0, r1, R, ldp);
        if (!live) continue;
        for (unsigned int r = 0; r < nr; ++r) {
            const double* x = ldp != 0u ? bpm_lds + r * ldp : H + (t0 + r) * ld;
            const double l = ln_like_point(x, d, y, (int)i, params);
            const bool first = acc.n == 0u;
            if (tr_add(acc, l)) {
                const BpmPwLse ms = bpm_pw_lse_add(first, m, s, l);
                m = ms.m; s = ms.s;
            } else if (l == l) {
                if (l > 0.0) ++n_pinf; else ++n_ninf;
            }
            if (values != nullptr) values[(t0 + r - lo) * n_data + i] = l;
        }
    }
    if (!live) return;
    const unsigned long long j = (unsigned long long)part * n_data + i;
    unsigned long long* u = reinterpret_cast<unsigned long long*>(rec);
    u[PW_N * n_rec + j] = acc.n;
    rec[PW_C * n_rec + j] = acc.c;
    rec[PW_S1 * n_rec + j] = acc.s1;
    rec[PW_S2 * n_rec + j] = acc.s2;
    u[PW_NAN * n_rec + j] = acc.n_nan;
    u[PW_PINF * n_rec + j] = n_pinf;
    u[PW_NINF * n_rec + j] = n_ninf;
    rec[PW_M * n_rec + j] = m;
    rec[PW_S * n_rec + j] = s;
}
#endif      // BPM_POINTWISE_W
