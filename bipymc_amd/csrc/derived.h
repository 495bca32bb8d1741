// Posterior summaries of a caller's DERIVED QUANTITIES: a function of one sample, given as HIP source, reduced over the window of the resident
// history where it lies.  The reference's fitting scripts end by taking param_est(n_burn)[2] to the host and running such a function over the
// samples (examples/ex_exp_fit.py:197-202: c_0 / c_inf per sample, its mean and standard deviation; :176-192: the fitted model at every sample
// for the trajectory picture; ex_line_fit.py and ex_para_fit.py likewise).  Here the caller writes
//     __device__ void derive(const double* x, int d, double ll, const double* p, double* out)
// (x: one super-chain row, d coordinates, never the padding column; ll: that row's stored ln-like; p: the caller's parameter block; out[0 .. n_out):
// zero on entry) and the library compiles ONE window-reduction kernel around it (hiprtc, as user_likelihood.h does for ln_like): per output the
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
#pragma once
#include "user_likelihood.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {

constexpr int DERIVE_THREADS = 256;
constexpr int DERIVE_MAX_OUT = 256;
constexpr int DERIVE_LDS_BYTES = USER_EVAL_LDS_BYTES;
constexpr int DERIVE_ACC_BYTES = 48;      // sizeof(TrAcc): the merge tree needs DERIVE_THREADS of them (static_assert in the wrapper)

inline const char* derive_wrapper() {
    return "\ntypedef unsigned int uint32_t; typedef unsigned long uint64_t;\n"
           "#define BPM_VARIANT_NS derived\n"
           "#include \"trace_acc.h\"\n"
           "extern \"C\" __global__ void __launch_bounds__(256) bpm_derive_rows(const double* H, const double* LL, unsigned int ld, int d, unsigned long long lo,\n"
           "                                                                  unsigned long long hi, const double* params, unsigned int n_out, unsigned int R,\n"
           "                                                                  unsigned int ldp, unsigned int ldo, double* rec, unsigned long long n_rec, double* values) {\n"
           "    using namespace bpm;\n"
           "    static_assert(sizeof(TrAcc) == 48, \"the host sizes the merge tree by 48 bytes per accumulator\");\n"
           "    extern __shared__ __attribute__((aligned(16))) double bpm_lds[];\n"
           "    double* const s_ll = bpm_lds + (unsigned long long)R * ldp;\n"
           "    double* const s_out = s_ll + R;\n"
           "    const unsigned int tid = threadIdx.x, cpw = 256u / n_out, m = tid % n_out, a = tid / n_out;\n"
           "    const unsigned long long chunk = (hi - lo + gridDim.x - 1) / gridDim.x;\n"
           "    unsigned long long r0 = lo + (unsigned long long)blockIdx.x * chunk;\n"
           "    r0 = r0 < hi ? r0 : hi;\n"
           "    const unsigned long long r1 = r0 + chunk < hi ? r0 + chunk : hi;\n"
           "    typedef double bpm_d2 __attribute__((ext_vector_type(2)));\n"
           "    TrAcc acc;\n"
           "    tr_init(acc);\n"
           "    for (unsigned long long t0 = r0; t0 < r1; t0 += R) {\n"
           "        const unsigned int nr = (unsigned int)(r1 - t0 < R ? r1 - t0 : R);\n"
           "        if (ldp != 0u) {\n"
           "            // pair k of the region -> row k / (ld / 2), 8 pairs per thread in flight\n"
           "            const bpm_d2* src = (const bpm_d2*)(H + t0 * ld);\n"
           "            const unsigned int h = ld >> 1, total = nr * h;\n"
           "            for (unsigned int k0 = 0; k0 < total; k0 += 256u * 8u) {\n"
           "                bpm_d2 v[8];\n"
           "#pragma unroll\n"
           "                for (int u = 0; u < 8; ++u) { const unsigned int k = k0 + u * 256u + tid; v[u] = src[k < total ? k : total - 1u]; }\n"
           "#pragma unroll\n"
           "                for (int u = 0; u < 8; ++u) {\n"
           "                    const unsigned int k = k0 + u * 256u + tid;\n"
           "                    if (k < total) {\n"
           "                        const unsigned int r = k / h, j = 2u * (k - r * h);\n"
           "                        if (j < (unsigned int)d) bpm_lds[r * ldp + j] = v[u].x;\n"
           "                        if (j + 1u < (unsigned int)d) bpm_lds[r * ldp + j + 1u] = v[u].y;\n"
           "                    }\n"
           "                }\n"
           "            }\n"
           "        }\n"
           "        if (tid < nr) s_ll[tid] = LL[t0 + tid];\n"
           "        __syncthreads();\n"
           "        if (tid < nr) {\n"
           "            double* o = s_out + tid * ldo;\n"
           "            for (unsigned int q = 0; q < n_out; ++q) o[q] = 0.0;\n"
           "            derive(ldp != 0u ? bpm_lds + tid * ldp : H + (t0 + tid) * ld, d, s_ll[tid], params, o);\n"
           "        }\n"
           "        __syncthreads();\n"
           "        if (a < cpw)\n"
           "            for (unsigned int r = a; r < nr; r += cpw) tr_add(acc, s_out[r * ldo + m]);\n"
           "        if (values != nullptr) {\n"
           "            double* dst = values + (t0 - lo) * n_out;\n"
           "            for (unsigned int i = tid; i < nr * n_out; i += 256u) { const unsigned int r = i / n_out; dst[i] = s_out[r * ldo + (i - r * n_out)]; }\n"
           "        }\n"
           "    }\n"
           "    __syncthreads();\n"
           "    TrAcc* s_acc = reinterpret_cast<TrAcc*>(bpm_lds);\n"
           "    s_acc[tid] = acc;\n"
           "    __syncthreads();\n"
           "    unsigned int top = 1u;\n"
           "    while (top < cpw) top <<= 1;\n"
           "    for (unsigned int s = top >> 1; s > 0u; s >>= 1) {      // the cpw lanes of an output: a halving tree, the same pairs every time\n"
           "        if (a < s && a + s < cpw) tr_merge(s_acc[tid], s_acc[tid + s * n_out]);\n"
           "        __syncthreads();\n"
           "    }\n"
           "    if (a == 0u) tr_store(rec, n_rec, (unsigned long long)blockIdx.x * n_out + m, s_acc[tid]);\n"
           "}\n";
}

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

// caller's source + wrapper -> code object for `arch`.  -> "" and `code`, or the reason (compiler log included).  trace_acc_h: the accumulator's
// header as the library carries it (embedded_src.h).  Compiled like ln_like: -O3 -ffp-contract=off.
inline std::string compile_device_function(Hiprtc& h, const std::string& user_src, const std::string& arch, const char* trace_acc_h, std::vector<char>& code) {
    const std::string why = load_hiprtc(h);
    if (!why.empty()) return why;
    static const char* prelude =
        "#ifndef INFINITY\n#define INFINITY (__builtin_huge_val())\n#endif\n"
        "#ifndef NAN\n#define NAN (__builtin_nan(\"\"))\n#endif\n"
        "#ifndef M_PI\n#define M_PI 3.14159265358979323846\n#endif\n"
        "#line 1 \"derive.hip\"\n";
    const std::string src = prelude + user_src + derive_wrapper();
    const char* hdr_src[] = {trace_acc_h};
    const char* hdr_names[] = {"trace_acc.h"};
    void* prog = nullptr;
    if (h.CreateProgram(&prog, src.c_str(), "derive.hip", 1, hdr_src, hdr_names) != 0 || !prog) return "hiprtcCreateProgram failed";
    const std::string a = "--offload-arch=" + arch;
    const char* opts[] = {a.c_str(), "-O3", "-ffp-contract=off"};
    const int rc = h.CompileProgram(prog, 3, opts);
    std::string log;
    size_t n = 0;
    if (h.GetProgramLogSize(prog, &n) == 0 && n > 1) {
        log.resize(n);
        if (h.GetProgramLog(prog, &log[0]) != 0) log.clear();
        while (!log.empty() && (log.back() == '\0' || log.back() == '\n')) log.pop_back();
    }
    if (rc != 0) {
        h.DestroyProgram(&prog);
        return "the function source does not compile (it must define `__device__ void derive(const double* x, int d, double ll, const double* p, double* out)`):\n" + log;
    }
    size_t sz = 0;
    if (h.GetCodeSize(prog, &sz) != 0 || sz == 0) { h.DestroyProgram(&prog); return "hiprtcGetCodeSize failed"; }
    code.resize(sz);
    const int rg = h.GetCode(prog, code.data());
    h.DestroyProgram(&prog);
    if (rg != 0) return "hiprtcGetCode failed";
    return "";
}

}  // namespace BPM_VARIANT_NS
}  // namespace bpm
