// DEVICE CODE OF A RUN-TIME PROGRAM (hiprtc; user_likelihood.h: user_fused_program includes it behind kernels.h and the caller's source).
// The caller's likelihood as a target of the library's own update kernel.  Target<TARGET_USER>::eval: the lanes of a chain put their coordinates
// of the row into LDS, the chain's first lane calls ln_like on it, the value goes back to the chain's lanes; in the per-coordinate form every lane
// adds the terms of its own coordinates and the kernel's reduction tree adds the lanes.  BPM_USER_LDP / BPM_USER_DIM: #defined by the program
// (the sampler's dimension is fixed, so the caller's loops over d get a compile-time trip count).
#include "user_ln_like.h"
namespace bpm { inline namespace BPM_VARIANT_NS {
constexpr int TARGET_USER = 64;
template <int LPC, int DPL>
struct Target<TARGET_USER, LPC, DPL> {
    struct Consts { const double* tp; };
    static __device__ __forceinline__ Consts load(int, uint32_t, const double* tp) { Consts k; k.tp = tp; return k; }
    static __device__ __forceinline__ double eval(const double* v, int q, uint32_t dim, const Consts& k) {
#ifdef BPM_LN_LIKE_TERMS
        // the per-coordinate form: every lane adds the terms of its own coordinates, the kernel's reduction tree adds the lanes
        double acc[BPM_LN_LIKE_TERMS];
#pragma unroll
        for (int t = 0; t < BPM_LN_LIKE_TERMS; ++t) acc[t] = 0.0;
#pragma unroll
        for (int s = 0; s < DPL; ++s) {
            const uint32_t j = 2u * (uint32_t)(q + (s >> 1) * LPC) + (uint32_t)(s & 1);
            if (j < dim) ::ln_like_terms(v[s], (int)j, BPM_USER_DIM, k.tp, acc);
        }
#pragma unroll
        for (int t = 0; t < BPM_LN_LIKE_TERMS; ++t) acc[t] = gsum<LPC>(acc[t]);
        return (double)::ln_like_finish(acc, BPM_USER_DIM, k.tp);
#else
        if (LPC == 1) return (double)::ln_like(v, BPM_USER_DIM, k.tp);      // (a lane is a chain: the row is the lane's registers)
        __shared__ double rows[(block_for_hot(LPC, 3, DPL) / LPC) * BPM_USER_LDP];      // (the burn-in flavours' workgroups hold the most chains)
        const int cw = (int)threadIdx.x / LPC;
        double* row = rows + cw * BPM_USER_LDP;
#pragma unroll
        for (int s = 0; s < DPL; ++s) {
            const uint32_t j = 2u * (uint32_t)(q + (s >> 1) * LPC) + (uint32_t)(s & 1);
            if (j < dim) row[j] = v[s];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double r = 0.0;
        if (q == 0) r = (double)::ln_like(row, BPM_USER_DIM, k.tp);
        if (LPC == WAVE) r = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(r)), __builtin_amdgcn_readfirstlane(__double2loint(r)));
        else if (LPC > 1) r = __shfl(r, (((int)threadIdx.x & (WAVE - 1)) / LPC) * LPC);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        return r;
#endif
    }
};
}}
