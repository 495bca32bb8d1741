// Microbenchmark (diagnostic): the FP64 matrix rate of v_mfma_f64_16x16x4_f64 from registers alone -- the compute bound of the covariance
// kernel (bipymc_amd/csrc/covariance.h, tools/covariance_time.py).  Every wavefront runs `iters` rounds of 28 independent accumulate
// chains (the kernel's 28 tile pairs at d = 100) on operands it never reloads; 2048 FLOP per instruction.  One wavefront per SIMD (1024
// workgroups of 64) and two (2048) are timed, each over a short and a long run.
//   hipcc -O3 --offload-arch=gfx950 -o build_variants/mfma_f64_rate tools/micro/mfma_f64_rate.hip && ./build_variants/mfma_f64_rate
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int CHAINS = 28;
__global__ __launch_bounds__(64) void k(double* out, int iters, double seed) {
    d4 acc[CHAINS];
    double a[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) a[t] = seed * (double)(threadIdx.x + t);
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[c % 7], a[(c * 3) % 7], acc[c], 0, 0, 0);
    }
    d4 s = acc[0];
#pragma unroll
    for (int c = 1; c < CHAINS; ++c) s += acc[c];
    out[(size_t)blockIdx.x * 64 + threadIdx.x] = s[0] + s[1] + s[2] + s[3];
}
int main() {
    hipStream_t st; (void)hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    double* out; (void)hipMalloc(&out, 4096 * 64 * sizeof(double));
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    // (1024 wavefronts = one per SIMD, 2048 = two; short and long runs: the sustained rate of a long run is lower than that of a run as
    // short as the covariance kernel's)
    const int cases[4][2] = {{1024, 1500}, {2048, 750}, {1024, 6000}, {2048, 3000}};
    for (const auto& cs : cases) {
        const int wg = cs[0], iters = cs[1];
        std::vector<float> ms;
        for (int rep = 0; rep < 7; ++rep) {        // the first two are warm-up
            (void)hipEventRecord(e0, st);
            hipLaunchKernelGGL(k, dim3(wg), dim3(64), 0, st, out, iters, 1e-9);
            (void)hipEventRecord(e1, st);
            (void)hipEventSynchronize(e1);
            float t; (void)hipEventElapsedTime(&t, e0, e1);
            if (rep >= 2) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        const double flop = (double)wg * iters * CHAINS * 2048.0;
        printf("mfma_f64_16x16x4 register-only: %d wavefronts x %d x %d instructions: %.3f ms (median of 5), %.2f TFLOP/s FP64\n", wg, iters, CHAINS,
               ms[2], flop / (ms[2] * 1e-3) / 1e12);
    }
    if (hipGetLastError() != hipSuccess) { printf("error\n"); return 1; }
    return 0;
}
