// The Metropolis accept test (samplers.py:328-336) without a full exp() on the path almost every update takes.
//
// An update uses two BITS of   alpha = clip(min(1, exp(d)), 0, 1),  d = (ll_prop + log_corr) - ll_cur :
//   accepted = !isnan(alpha) && u < alpha      and      isnan(alpha)   (the sampler's NaN counter);
// alpha itself is stored nowhere but in the test variant's decision trace (accept_alpha below).  A 53-bit exp() is needed for the first bit
// only when u falls inside the error of a cheaper exp(d).  accept_filter decides from a float32 2^t (ONE v_exp_f32 on the device) and says
// so when it cannot; accept_test then takes the plain formula, accept_exact, behind a branch.  The decision is that of accept_exact for
// EVERY (d, u): the filter's margins are set by the worst-case error of its route, not by how u is drawn.
//
//   d is NaN            is_nan, not accepted (exp gives NaN for NaN only)
//   d >= 0              exp(d) >= 1, the clamp is exactly 1: accepted = u < 1.0
//   d < D_LO = -40      exp(d) < exp(-40) = 4.25e-18 < 2^-53 (the smallest non-zero u01_53): not accepted when u >= 2^-53; a smaller u (0 in the
//                       sampler: a denormal exp(d) > 0 accepts there) goes to the plain formula
//   D_LO <= d < 0       e = (double)exp2_f32((float)(d * log2(e))); u < e (1 - DELTA): accepted; u >= e (1 + DELTA): not; between: plain formula.
//                       DELTA = 2^-12.  Error of e against the library's f64 exp(d): rounding t to float 2^-24 |t| ln 2 <= 2^-24 * 57.8 * 0.694 = 2.4e-6,
//                       v_exp_f32 1 ulp = 1.2e-7, the f64 product and the library's exp an ulp of f64 each: 2.6e-6 = DELTA / 94 (measured on the
//                       device: tests/test_gpu_accept_filter.py, which holds it under DELTA / 16).  t >= -57.8: e is a normal float.
//                       A random u lands between the bounds with probability 2 DELTA e <= 2 DELTA.
//
// __host__ __device__: the host flavour (exp2f / std::exp) states the same decisions in a plain C++ program (tests/test_accept_filter_host.py).
// -DBPM_ACCEPT_EXACT: accept_test is the plain formula only (timing builds: make variant NAME=... DEFS=-DBPM_ACCEPT_EXACT).
#pragma once
#if !defined(__HIPCC_RTC__) && !defined(__HIP_DEVICE_COMPILE__)
#include <math.h>
#endif

#if defined(__HIPCC__)
#define BPM_ACCEPT_HD __host__ __device__ __forceinline__
#else
#define BPM_ACCEPT_HD inline
#endif

namespace bpm {

constexpr double ACCEPT_D_LO = -40.0;
constexpr double ACCEPT_DELTA = 0x1p-12;
constexpr double ACCEPT_U_MIN = 0x1p-53;      // the smallest non-zero u01_53

// 2^t in float32: the hardware instruction on the device (the library's exp2f wraps denormal handling around it, which t >= -57.8 never needs)
BPM_ACCEPT_HD float accept_exp2_f32(float t) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(t);
#else
    return exp2f(t);
#endif
}

// the float32 route to exp(d): t = d log2(e) in f64, rounded to float, 2^t
BPM_ACCEPT_HD double accept_route(double d) {
    const double t = d * 1.4426950408889634;             // log2(e)
    return (double)accept_exp2_f32((float)t);
}

// today's four lines: the value the trace records ...
BPM_ACCEPT_HD double accept_alpha(double d, bool* is_nan) {
    double alpha = exp(d);
    *is_nan = alpha != alpha;
    alpha = fmin(1.0, alpha);
    alpha = fmax(0.0, alpha);                            // np.clip(np.min((1, .)), 0, 1); NaN stays NaN in NumPy
    return alpha;
}
// ... and the decision taken from it
BPM_ACCEPT_HD bool accept_exact(double d, double u, bool* is_nan) {
    const double alpha = accept_alpha(d, is_nan);
    return !*is_nan && (u < alpha);
}

// What the float32 route says: yes = accepted, ask = it cannot decide (neither: not accepted; d NaN: is_nan, neither).  Straight-line on purpose -- the
// classes are combined as bits, so that a wavefront-uniform d costs compares and scalar mask operations, not a chain of branches.
BPM_ACCEPT_HD void accept_filter(double d, double u, bool* yes, bool* ask, bool* is_nan) {
    const double e = accept_route(d);
    const bool yes_mid = u < e * (1.0 - ACCEPT_DELTA), no_mid = u >= e * (1.0 + ACCEPT_DELTA);
    const bool nan = d != d, nonneg = d >= 0.0, ge_lo = d >= ACCEPT_D_LO;
    const bool mid = ge_lo & !nonneg, far = !ge_lo & !nan;
    *yes = (nonneg & (u < 1.0)) | (mid & yes_mid);
    *ask = (far & !(u >= ACCEPT_U_MIN)) | (mid & !(yes_mid | no_mid));
    *is_nan = nan;
}

BPM_ACCEPT_HD bool accept_test(double d, double u, bool* is_nan) {
#ifdef BPM_ACCEPT_EXACT
    return accept_exact(d, u, is_nan);
#else
    bool accepted, ask;
    accept_filter(d, u, &accepted, &ask, is_nan);
    if (ask) {      // (one wavefront per chain: uniform; several chains per wavefront: taken when any lane asks)
        bool nan_exact;
        accepted = accept_exact(d, u, &nan_exact);
    }
    return accepted;
#endif
}

}   // namespace bpm
