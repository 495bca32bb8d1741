// DEVICE CODE OF A RUN-TIME PROGRAM (hiprtc; user_likelihood.h: compile_user_likelihood includes it behind the caller's source).
// The kernel around the caller's function: work item i of a half generation (row i of `rows`, stride ld) -> out[i]; an inactive work item (ids[i] < 0:
// a rank of a world launches one item per local chain and half of them sit in the other pool) is not evaluated.  ids == nullptr: every row.
// A workgroup of 64 threads takes `rpb` consecutive rows: it copies them -- contiguous in memory, so the loads coalesce -- into LDS (row stride ldp
// doubles, odd: the threads' column reads spread over the banks), then thread r calls the caller's function on row r in LDS.  A thread per row reading
// its row straight from memory (stride 800 B between the lanes at d = 100) took 15.6 us for 4096 rows; staged: see profiles/r05_hip_source_likelihood.txt.
// rpb == 0 (rows too wide for a useful tile): every thread reads its row where it lies.
// The host's view of the parameter list: user_likelihood.h, UserEvalKernel.
#include "user_ln_like.h"

extern "C" __global__ void __launch_bounds__(64) bpm_user_eval(const double* rows, const int* ids, int n, int ld, int d, const double* params,
                                                              double* out, int rpb, int ldp) {
    extern __shared__ double bpm_tile[];
    if (rpb == 0) {
        const int i = (int)(blockIdx.x * 64 + threadIdx.x);
        if (i < n) out[i] = (ids == nullptr || ids[i] >= 0) ? (double)ln_like(rows + (unsigned long long)i * (unsigned long long)ld, d, params) : 0.0;
        return;
    }
    const int r0 = (int)blockIdx.x * rpb;
    const int nr = (n - r0) < rpb ? (n - r0) : rpb;
    // the workgroup's nr rows lie back to back (ld even: 16-byte pairs): pair k of the region -> row k / (ld / 2), 8 pairs per thread in flight
    typedef double bpm_d2 __attribute__((ext_vector_type(2)));
    const bpm_d2* src = (const bpm_d2*)(rows + (unsigned long long)r0 * (unsigned long long)ld);
    const int h = ld >> 1, total = nr * h;
    for (int k0 = 0; k0 < total; k0 += 64 * 8) {
        bpm_d2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = k0 + u * 64 + (int)threadIdx.x; v[u] = src[k < total ? k : total - 1]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + u * 64 + (int)threadIdx.x;
            if (k < total) { const int r = k / h, j = 2 * (k - r * h); bpm_tile[r * ldp + j] = v[u].x; if (j + 1 < d) bpm_tile[r * ldp + j + 1] = v[u].y; }
        }
    }
    __syncthreads();
    const int t = (int)threadIdx.x;
    if (t < nr) out[r0 + t] = (ids == nullptr || ids[r0 + t] >= 0) ? (double)ln_like(bpm_tile + t * ldp, d, params) : 0.0;
}
