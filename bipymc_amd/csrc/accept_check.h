// Device self-test of the accept test (accept_test.h): its decisions against the plain formula with the device library's exp(), and the measured
// error of its float32 route -- the hardware's v_exp_f32, which no host program can stand in for.  Used by bpm_selftest_accept /
// bpm_selftest_accept_error (tests/test_gpu_accept_filter.py) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "accept_test.h"
#include "philox.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {      // (philox.h: one kernel-symbol namespace per build variant)

// out: five bytes per case -- accept_test's decision, the plain formula's, accept_test's NaN flag, the plain formula's, "the filter asked for the exact path"
__global__ void accept_check_kernel(int n, const double* d, const double* u, uint8_t* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double di = d[i], ui = u[i];
    bool nan_t, nan_f, yes, ask;
    const bool acc = accept_test(di, ui, &nan_t);
    accept_filter(di, ui, &yes, &ask, &nan_f);
    double alpha = exp(di);
    const bool nan_p = alpha != alpha;
    alpha = fmin(1.0, alpha);
    alpha = fmax(0.0, alpha);
    uint8_t* o = out + 5 * (size_t)i;
    o[0] = acc ? 1 : 0; o[1] = (!nan_p && ui < alpha) ? 1 : 0; o[2] = nan_t ? 1 : 0; o[3] = nan_p ? 1 : 0; o[4] = ask ? 1 : 0;
}

// (a non-negative double's bit pattern orders as the value does)
__device__ __forceinline__ void accept_err_max(double err, unsigned long long* slot) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) err = fmax(err, __shfl_xor(err, m));
    if ((threadIdx.x & 63) == 0) atomicMax(slot, (unsigned long long)__double_as_longlong(err));
}

// every float t = -|t| with bit pattern bits_lo <= bits(|t|) <= bits_hi: | (double)exp2_f32(t) / exp2_f64(t) - 1 |, the maximum into *slot
__global__ void accept_exp2_sweep_kernel(uint32_t bits_lo, uint32_t bits_hi, unsigned long long* slot) {
    double worst = 0.0;
    const uint64_t n = (uint64_t)bits_hi - bits_lo + 1u, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float t = -__uint_as_float(bits_lo + (uint32_t)i);
        const double e = (double)accept_exp2_f32(t);
        worst = fmax(worst, fabs(e / exp2((double)t) - 1.0));
    }
    accept_err_max(worst, slot);
}

// the whole route of accept_filter, d -> t = d log2(e) -> float -> 2^t, against the library's exp(d): the maximum relative difference into *slot
__global__ void accept_route_kernel(int n, const double* d, unsigned long long* slot) {
    double worst = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        worst = fmax(worst, fabs(accept_route(d[i]) / exp(d[i]) - 1.0));
    }
    accept_err_max(worst, slot);
}

}  // inline namespace BPM_VARIANT_NS
}  // namespace bpm
