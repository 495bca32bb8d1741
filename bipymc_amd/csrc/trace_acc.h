// The shifted, order-fixed accumulator of the trace summaries (traces.h) and of the derived quantities (derived.h): its one definition.
// No includes: the library's translation unit reaches it through traces.h (behind kernels.h), a program compiled at run time around a
// caller's function gets it as an embedded header (embedded_src.h) behind the fixed-width typedefs and BPM_VARIANT_NS of its own.
//
// Over the finite values: their count n, a shift c (the first finite value the accumulator met) and S1 = sum (x - c), S2 = sum (x - c)^2;
// how many values are NaN; min and max over the values that are not NaN.  traces.h says why and how they merge.
#pragma once

namespace bpm {
inline namespace BPM_VARIANT_NS {

// fields of a record: the first TR_F_BINS of every record, all TR_F_LL of a ln-like record
enum { TR_N = 0, TR_C, TR_S1, TR_S2, TR_NAN, TR_MIN, TR_MAX, TR_F_BINS, TR_PINF = TR_F_BINS, TR_NINF, TR_BKEY, TR_BROW, TR_F_LL };

struct TrAcc {
    double c, s1, s2, mn, mx;
    uint32_t n, n_nan;                         // (a workgroup sees fewer than 2^31 rows: the host sizes the parts so)
};

__device__ __forceinline__ void tr_init(TrAcc& a) {
    a.c = a.s1 = a.s2 = 0.0;
    a.mn = __longlong_as_double(0x7FF0000000000000ll);
    a.mx = -a.mn;
    a.n = a.n_nan = 0u;
}

// -> x is finite and went into the moments
__device__ __forceinline__ bool tr_add(TrAcc& a, double x) {
    if (x != x) { ++a.n_nan; return false; }
    a.mn = x < a.mn ? x : a.mn;
    a.mx = x > a.mx ? x : a.mx;
    if (x - x != 0.0) return false;
    if (a.n == 0u) a.c = x;
    const double d = x - a.c;
    a.s1 += d;
    a.s2 += d * d;
    ++a.n;
    return true;
}

template <class Count>
__device__ __forceinline__ void tr_merge_moments(Count& n, double& c, double& s1, double& s2, Count nb, double cb, double s1b, double s2b) {
    if (nb == 0) return;
    if (n == 0) { n = nb; c = cb; s1 = s1b; s2 = s2b; return; }
    const double d = cb - c, w = (double)nb;
    s1 += s1b + w * d;
    s2 += s2b + (2.0 * d * s1b + w * d * d);
    n += nb;
}

__device__ __forceinline__ void tr_merge(TrAcc& a, const TrAcc& b) {
    tr_merge_moments(a.n, a.c, a.s1, a.s2, b.n, b.c, b.s1, b.s2);
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    a.n_nan += b.n_nan;
}

__device__ __forceinline__ void tr_store(double* __restrict__ rec, uint64_t n_rec, uint64_t j, const TrAcc& a) {
    unsigned long long* u = reinterpret_cast<unsigned long long*>(rec);
    u[TR_N * n_rec + j] = a.n;
    rec[TR_C * n_rec + j] = a.c;
    rec[TR_S1 * n_rec + j] = a.s1;
    rec[TR_S2 * n_rec + j] = a.s2;
    u[TR_NAN * n_rec + j] = a.n_nan;
    rec[TR_MIN * n_rec + j] = a.mn;
    rec[TR_MAX * n_rec + j] = a.mx;
}

}  // inline namespace BPM_VARIANT_NS
}  // namespace bpm
