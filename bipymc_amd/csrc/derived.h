// Posterior summaries of a caller's DERIVED QUANTITIES: a function of one sample, given as HIP source, reduced over the window of the resident
// history where it lies.  The reference's fitting scripts end by taking param_est(n_burn)[2] to the host and running such a function over the
// samples (examples/ex_exp_fit.py:197-202: c_0 / c_inf per sample, its mean and standard deviation; :176-192: the fitted model at every sample
// for the trajectory picture; ex_line_fit.py and ex_para_fit.py likewise).  Here the caller writes
//     __device__ void derive(const double* x, int d, double ll, const double* p, double* out)
// (x: one super-chain row, d coordinates, never the padding column; ll: that row's stored ln-like; p: the caller's parameter block; out[0 .. n_out):
// zero on entry) and the library compiles a window-reduction kernel around it (hiprtc, as user_likelihood.h does for ln_like): per output the
// count, shift and shifted sums of the finite values, the NaN count, min and max -- trace_acc.h's accumulator, merged in a fixed order without
// atomics -- and, if asked, the values themselves.  bipymc_amd/derived.py merges the ranks and finishes mean and sd.
//
//   bpm_derive_rows   grid (parts): workgroup p takes the rows [lo + p chunk, min(lo + (p + 1) chunk, hi)), chunk = ceil((hi - lo) / parts), in
//                     tiles of R rows.  Per tile, two barriers between three steps:
//                       1. stage   the tile's rows lie back to back (ld even: 16-byte pairs): 256 threads copy them into LDS with 8 16-byte loads
//                                  each in flight, row stride ldp = d | 1 doubles (odd: the threads' column reads spread over the banks); the R
//                                  ln-likes go beside them.  ldp == 0 (rows too wide for a useful tile): no copy, x points at the row in memory.
//                       2. call    thread r < R zeroes its n_out slots of the LDS output tile (row stride ldo = n_out | 1) and calls derive on
//                                  row r: the caller's `out` is LDS, the wrapper holds no per-thread array.
//                       3. add     thread (a, m), m = tid % n_out, a = tid / n_out < cpw = 256 / n_out, adds output m of the tile's rows
//                                  a, a + cpw, ... to its accumulator, rows ascending; with `values` the tile goes out as it lies in LDS,
//                                  values[(row - lo) * n_out + m], consecutive m on consecutive lanes.
//                     After the last tile the cpw lanes of an output merge by the halving tree of tr_bins_kernel and lane (0, m) stores part
//                     record p * n_out + m (traces.h's structure of arrays, one bin, ld := n_out); the library's tr_fold_kernel folds the
//                     parts in index order.  LDS is dynamic only: [rows R x ldp | ln-likes R | outputs R x ldo], and the merge tree's 256
//                     accumulators over the same bytes afterwards.
//   bpm_derive_fill   the DERIVED HISTORY (bpm_derive_history): the same grid over ALL local rows [0, hist_rows * n_local), the same steps 1 and 2
//                     (derive_rows.h: bpm_derive_tile, the one staging routine of both kernels), and instead of step 3
//                       3. store   the output tile leaves LDS straight into the history buffer D of a second, ordinary handle with dim = n_out:
//                                  D[(t0 + r) * ldd + m] = m < n_out ? out[r][m] : 0 for m < ldd, ldd that handle's (even) row stride -- the
//                                  padding column is written as 0, as bpm_set_history leaves it.  The tile's destination is contiguous:
//                                  consecutive lanes store consecutive 16-byte pairs.
//                     No accumulators, no merge tree.  Every statistic of the history (bpm_reduce_moments ... bpm_trace_chains, bpm_derive
//                     itself) then serves the derived quantities through that handle, unchanged.
#pragma once
#include "user_likelihood.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {

constexpr int DERIVE_THREADS = 256;
constexpr int DERIVE_MAX_OUT = 256;
constexpr int DERIVE_LDS_BYTES = USER_EVAL_LDS_BYTES;
constexpr int DERIVE_ACC_BYTES = 48;      // sizeof(TrAcc): the merge tree needs DERIVE_THREADS of them (static_assert in the wrapper)

// bpm_derive_rows (derive_rows.h: device code, compiled at run time only) as the host launches it: H, LL, ld, d, lo, hi, params, n_out, R, ldp, ldo,
// rec, n_rec, values
using DeriveRowsKernel = void(const double*, const double*, unsigned int, int, unsigned long long, unsigned long long, const double*, unsigned int, unsigned int,
                              unsigned int, unsigned int, double*, unsigned long long, double*);
// bpm_derive_fill likewise: H, LL, ld, d, n_rows, params, n_out, R, ldp, ldo, D, ldd
using DeriveFillKernel = void(const double*, const double*, unsigned int, int, unsigned long long, const double*, unsigned int, unsigned int, unsigned int,
                              unsigned int, double*, unsigned int);

// rows per tile R, the LDS strides (ldp == 0: rows are read where they lie) and the dynamic LDS of a launch, for rows of d coordinates and n_out outputs
inline void derive_tile(uint32_t d, uint32_t n_out, uint32_t budget_bytes, uint32_t& R, uint32_t& ldp, uint32_t& ldo, uint32_t& lds_bytes) {
    const uint32_t budget = budget_bytes / 8u;      // doubles
    ldo = n_out | 1u;
    ldp = d | 1u;
    uint32_t rows = budget / (ldp + 1u + ldo);
    if (rows < 16u) {      // wide rows: the output tile alone
        ldp = 0u;
        rows = budget / (1u + ldo);
    }
    R = rows < (uint32_t)DERIVE_THREADS ? rows : (uint32_t)DERIVE_THREADS;
    const uint32_t tiles = R * (ldp + 1u + ldo) * 8u, tree = (uint32_t)(DERIVE_THREADS * DERIVE_ACC_BYTES);
    lds_bytes = ((tiles > tree ? tiles : tree) + 15u) & ~15u;
}

// caller's source + wrapper -> code object for `arch`.  -> "" and `code`, or the reason (compiler log included).  headers: the library's embedded
// files, derive_rows.h and the accumulator's trace_acc.h among them.  Compiled like ln_like: -O3 -ffp-contract=off.
inline std::string compile_device_function(const std::string& user_src, const std::string& arch, const RtcHeader* headers, size_t n_headers, std::vector<char>& code) {
    const std::string src = std::string(RTC_PRELUDE) + "#line 1 \"derive.hip\"\n" + user_src + "\n#include \"derive_rows.h\"\n";
    return rtc_compile(src, "derive.hip", headers, n_headers, arch, {},
                       "the function source does not compile (it must define `__device__ void derive(const double* x, int d, double ll, const double* p, double* out)`):\n", code);
}

}  // namespace BPM_VARIANT_NS
}  // namespace bpm
