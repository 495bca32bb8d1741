// DEVICE CODE OF A RUN-TIME PROGRAM (hiprtc; user_likelihood.h: compile_user_likelihood includes it behind a source in the PER-DATUM form).
// A likelihood that is a function of K sums over the caller's DATA (samplers.py:36-43 takes any callable; every fitting script of the reference sums
// (y - model)^2 over its data points inside it).  The source says
//     #define BPM_LN_LIKE_DATA K                    // number of accumulators, 1 ... 8        (HipLikelihood(data=..., terms=K) writes both)
//     #define BPM_LN_LIKE_DATA_W w                  // doubles per datum, 1 ... 64
//     __device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc)     // adds datum i (its w values: y) into acc[0 .. K)
//     __device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p)         // the value from the K sums (x: for a prior)
// and the data axis is the parallel one: a WAVEFRONT per (row, chunk), a chunk being BPM_DATA_CHUNK consecutive data points.
//
// THE ORDER OF THE ADDITIONS -- a function of n_data alone, so that a row's value depends on (x, data, params) and on nothing else: not on the number of
// rows of the launch, the row's place among them, the batch it fell into or the number of workgroups.
//   1. lane l of the wavefront of chunk c starts K accumulators at 0.0 and calls ln_like_datum on the data c C + l, c C + l + 64, ... below
//      min((c + 1) C, n_data), in increasing order (at most C / 64 calls);
//   2. the 64 lanes' accumulators meet in six butterfly levels, partner distance 32, 16, 8, 4, 2, 1 in that order: at every level a lane replaces its
//      value v by v + (the value of lane l ^ distance) -- IEEE addition commutes, so after the sixth level all 64 lanes hold the same bits;
//   3. n_data <= C: that is the row's sum.  Else the chunks' sums lie in `part` [row][chunk][K], and bpm_user_fold_data starts K accumulators at 0.0
//      and adds the chunks 0, 1, 2, ... in increasing order;
//   4. ln_like_total is called once per row on the K sums.
// The row x is copied once per wavefront into LDS when d <= BPM_DATA_XMAX (the workgroup's budget: BPM_DATA_WAVES x BPM_DATA_XMAX doubles = 16 KiB);
// a wider row is read where it lies, at a wave-uniform address.  The data are read (n_data, w) row-major: 64 lanes read 64 w consecutive doubles.
// Rows with ids[row] < 0 are not evaluated (out = 0.0), as in bpm_user_eval.  The host's view of the parameter lists: user_likelihood.h.
#define BPM_DATA_CHUNK 4096
#define BPM_DATA_WAVES 4
#define BPM_DATA_XMAX 512

#if BPM_LN_LIKE_DATA < 1 || BPM_LN_LIKE_DATA > 8
#error "BPM_LN_LIKE_DATA (the number of accumulators) must be 1 ... 8"
#endif
#if !defined(BPM_LN_LIKE_DATA_W) || BPM_LN_LIKE_DATA_W < 1 || BPM_LN_LIKE_DATA_W > 64
#error "BPM_LN_LIKE_DATA_W (doubles per datum) must be 1 ... 64"
#endif

// n_chunks = ceil(n_data / C), n_items = n * n_chunks wavefronts' worth of work (the host keeps it below 2^31: rows go in batches)
extern "C" __global__ void __launch_bounds__(64 * BPM_DATA_WAVES) bpm_user_eval_data(const double* rows, const int* ids, int n, int ld, int d, const double* params,
                                                                                      const double* data, int n_data, int n_chunks, double* out, double* part) {
    __shared__ double bpm_xs[BPM_DATA_WAVES][BPM_DATA_XMAX];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const long long item = (long long)blockIdx.x * BPM_DATA_WAVES + wave;
    const bool live = item < (long long)n * n_chunks;
    const int row = live ? (int)(item / n_chunks) : 0, chunk = live ? (int)(item - (long long)row * n_chunks) : 0;
    const bool active = live && (ids == nullptr || ids[row] >= 0);
    const double* x = rows + (unsigned long long)row * (unsigned long long)ld;
    if (d <= BPM_DATA_XMAX) {
        if (active) for (int j = lane; j < d; j += 64) bpm_xs[wave][j] = x[j];
        x = bpm_xs[wave];
    }
    __syncthreads();      // (every wavefront of the workgroup arrives, idle ones included; each reads only the row it wrote itself)
    if (!live) return;
    if (!active) { if (chunk == 0 && lane == 0) out[row] = 0.0; return; }
    double acc[BPM_LN_LIKE_DATA];
#pragma unroll
    for (int k = 0; k < BPM_LN_LIKE_DATA; ++k) acc[k] = 0.0;
    const long long i0 = (long long)chunk * BPM_DATA_CHUNK, i1 = (i0 + BPM_DATA_CHUNK) < (long long)n_data ? (i0 + BPM_DATA_CHUNK) : (long long)n_data;
    for (long long i = i0 + lane; i < i1; i += 64) ln_like_datum(x, d, data + (unsigned long long)i * BPM_LN_LIKE_DATA_W, (int)i, params, acc);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < BPM_LN_LIKE_DATA; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
    }
    if (lane != 0) return;
    if (n_chunks == 1) { out[row] = (double)ln_like_total(x, d, acc, n_data, params); return; }
    double* dst = part + (unsigned long long)item * BPM_LN_LIKE_DATA;
#pragma unroll
    for (int k = 0; k < BPM_LN_LIKE_DATA; ++k) dst[k] = acc[k];
}

// n_data > C: a thread per row adds the row's chunk sums in increasing chunk order and calls ln_like_total (rows with ids < 0 were given 0.0 above)
extern "C" __global__ void __launch_bounds__(64) bpm_user_fold_data(const double* rows, const int* ids, int n, int ld, int d, const double* params,
                                                                   const double* part, int n_data, int n_chunks, double* out) {
    const int row = (int)(blockIdx.x * 64 + threadIdx.x);
    if (row >= n || (ids != nullptr && ids[row] < 0)) return;
    double acc[BPM_LN_LIKE_DATA];
#pragma unroll
    for (int k = 0; k < BPM_LN_LIKE_DATA; ++k) acc[k] = 0.0;
    const double* src = part + (unsigned long long)row * (unsigned long long)n_chunks * BPM_LN_LIKE_DATA;
    for (int c = 0; c < n_chunks; ++c) {
#pragma unroll
        for (int k = 0; k < BPM_LN_LIKE_DATA; ++k) acc[k] += src[(unsigned long long)c * BPM_LN_LIKE_DATA + k];
    }
    out[row] = (double)ln_like_total(rows + (unsigned long long)row * (unsigned long long)ld, d, acc, n_data, params);
}

// what the host must agree with: K, w, C and the wavefronts per workgroup of THIS program
extern "C" __global__ void bpm_user_data_info(int* o) { o[0] = BPM_LN_LIKE_DATA; o[1] = BPM_LN_LIKE_DATA_W; o[2] = BPM_DATA_CHUNK; o[3] = BPM_DATA_WAVES; }
