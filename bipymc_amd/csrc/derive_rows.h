// DEVICE CODE OF A RUN-TIME PROGRAM (hiprtc; derived.h: compile_device_function includes it behind the caller's source).
// Two kernels around the caller's `derive`, sharing bpm_derive_tile -- stage a tile of rows in LDS, call derive per row:
//   bpm_derive_rows: the window reduction -- add the outputs into trace_acc.h's accumulators, merge by a halving tree;
//   bpm_derive_fill: the derived history -- the output tile leaves LDS straight into another handle's history buffer.
// derived.h describes the steps and the LDS layout, and holds the host's view of the parameter lists (DeriveRowsKernel, DeriveFillKernel).

typedef unsigned int uint32_t; typedef unsigned long uint64_t;
#define BPM_VARIANT_NS derived
#include "trace_acc.h"
typedef double bpm_d2 __attribute__((ext_vector_type(2)));

// Step 1 of a tile (derived.h), all 256 threads of the workgroup: the nr rows from local row t0 on into LDS at row stride ldp (odd, >= d).  No barrier.
// (pointwise_rows.h stages its rows with it too and takes nothing else of this file: BPM_STAGE_ROWS_ONLY.)
__device__ __forceinline__ void bpm_stage_rows(double* lds, const double* H, unsigned int ld, int d, unsigned long long t0, unsigned int nr, unsigned int ldp) {
    // pair k of the region -> row k / (ld / 2), 8 pairs per thread in flight
    const unsigned int tid = threadIdx.x;
    const bpm_d2* src = (const bpm_d2*)(H + t0 * ld);
    const unsigned int h = ld >> 1, total = nr * h;
    for (unsigned int k0 = 0; k0 < total; k0 += 256u * 8u) {
        bpm_d2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const unsigned int k = k0 + u * 256u + tid; v[u] = src[k < total ? k : total - 1u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const unsigned int k = k0 + u * 256u + tid;
            if (k < total) {
                const unsigned int r = k / h, j = 2u * (k - r * h);
                if (j < (unsigned int)d) lds[r * ldp + j] = v[u].x;
                if (j + 1u < (unsigned int)d) lds[r * ldp + j + 1u] = v[u].y;
            }
        }
    }
}

#ifndef BPM_STAGE_ROWS_ONLY
// Steps 1 and 2 of a tile (derived.h), all 256 threads of the workgroup: the nr <= R rows from local row t0 on into LDS (lds: the dynamic LDS,
// [rows R x ldp | ln-likes R | outputs R x ldo]), a barrier, thread r < nr calls derive on row r, a barrier.  -> the output tile (row stride ldo).
// The caller may read it until it calls this again.
__device__ __forceinline__ double* bpm_derive_tile(double* lds, const double* H, const double* LL, unsigned int ld, int d, unsigned long long t0,
                                                   unsigned int nr, const double* params, unsigned int n_out, unsigned int R, unsigned int ldp,
                                                   unsigned int ldo) {
    double* const s_ll = lds + (unsigned long long)R * ldp;
    double* const s_out = s_ll + R;
    const unsigned int tid = threadIdx.x;
    if (ldp != 0u) bpm_stage_rows(lds, H, ld, d, t0, nr, ldp);
    if (tid < nr) s_ll[tid] = LL[t0 + tid];
    __syncthreads();
    if (tid < nr) {
        double* o = s_out + tid * ldo;
        for (unsigned int q = 0; q < n_out; ++q) o[q] = 0.0;
        derive(ldp != 0u ? lds + tid * ldp : H + (t0 + tid) * ld, d, s_ll[tid], params, o);
    }
    __syncthreads();
    return s_out;
}

// the rows [r0, r1) of [lo, hi) that workgroup blockIdx.x of gridDim.x takes: chunk = ceil((hi - lo) / parts) rows each, the last ones fewer or none
__device__ __forceinline__ void bpm_derive_part(unsigned long long lo, unsigned long long hi, unsigned long long& r0, unsigned long long& r1) {
    const unsigned long long chunk = (hi - lo + gridDim.x - 1) / gridDim.x;
    r0 = lo + (unsigned long long)blockIdx.x * chunk;
    r0 = r0 < hi ? r0 : hi;
    r1 = r0 + chunk < hi ? r0 + chunk : hi;
}

extern "C" __global__ void __launch_bounds__(256) bpm_derive_rows(const double* H, const double* LL, unsigned int ld, int d, unsigned long long lo,
                                                                  unsigned long long hi, const double* params, unsigned int n_out, unsigned int R,
                                                                  unsigned int ldp, unsigned int ldo, double* rec, unsigned long long n_rec, double* values) {
    using namespace bpm;
    static_assert(sizeof(TrAcc) == 48, "the host sizes the merge tree by 48 bytes per accumulator");
    extern __shared__ __attribute__((aligned(16))) double bpm_lds[];
    const unsigned int tid = threadIdx.x, cpw = 256u / n_out, m = tid % n_out, a = tid / n_out;
    unsigned long long r0, r1;
    bpm_derive_part(lo, hi, r0, r1);
    TrAcc acc;
    tr_init(acc);
    for (unsigned long long t0 = r0; t0 < r1; t0 += R) {
        const unsigned int nr = (unsigned int)(r1 - t0 < R ? r1 - t0 : R);
        const double* s_out = bpm_derive_tile(bpm_lds, H, LL, ld, d, t0, nr, params, n_out, R, ldp, ldo);
        if (a < cpw)
            for (unsigned int r = a; r < nr; r += cpw) tr_add(acc, s_out[r * ldo + m]);
        if (values != nullptr) {
            double* dst = values + (t0 - lo) * n_out;
            for (unsigned int i = tid; i < nr * n_out; i += 256u) { const unsigned int r = i / n_out; dst[i] = s_out[r * ldo + (i - r * n_out)]; }
        }
    }
    __syncthreads();
    TrAcc* s_acc = reinterpret_cast<TrAcc*>(bpm_lds);
    s_acc[tid] = acc;
    __syncthreads();
    unsigned int top = 1u;
    while (top < cpw) top <<= 1;
    for (unsigned int s = top >> 1; s > 0u; s >>= 1) {      // the cpw lanes of an output: a halving tree, the same pairs every time
        if (a < s && a + s < cpw) tr_merge(s_acc[tid], s_acc[tid + s * n_out]);
        __syncthreads();
    }
    if (a == 0u) tr_store(rec, n_rec, (unsigned long long)blockIdx.x * n_out + m, s_acc[tid]);
}

// The local rows [0, n_rows) of H through derive into the history buffer D of another handle (row stride ldd: even, n_out or n_out + 1): no
// accumulators, no merge tree.  A tile's destination D[t0 * ldd .. (t0 + nr) * ldd) is contiguous and 16-byte aligned: pair k of it is row
// k / (ldd / 2), columns 2 (k % (ldd / 2)) and the next, consecutive lanes store consecutive pairs; a column >= n_out (the padding) is 0.
extern "C" __global__ void __launch_bounds__(256) bpm_derive_fill(const double* H, const double* LL, unsigned int ld, int d, unsigned long long n_rows,
                                                                  const double* params, unsigned int n_out, unsigned int R, unsigned int ldp,
                                                                  unsigned int ldo, double* D, unsigned int ldd) {
    extern __shared__ __attribute__((aligned(16))) double bpm_lds[];
    const unsigned int tid = threadIdx.x, hd = ldd >> 1;
    unsigned long long r0, r1;
    bpm_derive_part(0ull, n_rows, r0, r1);
    for (unsigned long long t0 = r0; t0 < r1; t0 += R) {
        const unsigned int nr = (unsigned int)(r1 - t0 < R ? r1 - t0 : R);
        const double* s_out = bpm_derive_tile(bpm_lds, H, LL, ld, d, t0, nr, params, n_out, R, ldp, ldo);
        bpm_d2* dst = (bpm_d2*)(D + t0 * ldd);
        for (unsigned int k = tid; k < nr * hd; k += 256u) {
            const unsigned int r = k / hd, j = 2u * (k - r * hd);
            const double* o = s_out + r * ldo + j;
            bpm_d2 v;
            v.x = j < n_out ? o[0] : 0.0;
            v.y = j + 1u < n_out ? o[1] : 0.0;
            dst[k] = v;
        }
    }
}
#endif      // BPM_STAGE_ROWS_ONLY
