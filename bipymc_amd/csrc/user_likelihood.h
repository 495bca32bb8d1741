// A caller's ln_like_fn given as HIP SOURCE (samplers.py:36-43 takes any Python callable): compiled at run time with hiprtc into ONE
// small kernel -- a thread per proposal row calls the caller's `ln_like` -- that runs between the library's own proposal and commit kernels
// (phase_propose_kernel / phase_commit_kernel, the kernels of the host-callback path).  Nothing leaves the device and no host code runs inside a
// generation: bpm_step drives such a sampler like one with a shipped target.  The update kernels themselves are not recompiled.
//
// What the caller writes (HIP device code; double precision; no includes needed):
//     __device__ double ln_like(const double* x, int d, const double* p)      // x: one parameter vector, p: the caller's parameter block
// (the device math functions, INFINITY, NAN and M_PI are there; a prior outside its support returns -INFINITY like a Python ln_like_fn would)
// The PER-COORDINATE form (optional; for likelihoods that are a function of a few sums over the coordinates): the source says
//     #define BPM_LN_LIKE_TERMS K                                                               // number of accumulators, <= 8
//     __device__ void ln_like_terms(double xj, int j, int d, const double* p, double* acc)       // adds coordinate j's contribution into acc[0 .. K)
//     __device__ double ln_like_finish(const double* acc, int d, const double* p)                // the value from the K sums
// and the library derives ln_like from them (user_ln_like_from_terms).  Inside the update kernel every lane of a chain then adds the terms of ITS
// coordinates and the sums meet in the kernel's own reduction tree -- the shape of the shipped targets -- where the plain form runs on one lane per chain.
// hiprtc is loaded on demand (libhiprtc.so): a process that never installs such a likelihood never needs it.
#pragma once
#include "rtc.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {

// The kernel around the caller's function is user_eval.h (device code, compiled at run time only); this is its parameter list as the host
// launches it -- rows, ids, n, ld, d, params, out, rpb, ldp -- and its launch geometry: 64 threads, `rpb` rows staged in LDS per workgroup.
using UserEvalKernel = void(const double*, const int*, int, int, int, const double*, double*, int, int);
constexpr int USER_EVAL_BLOCK = 64;
constexpr int USER_EVAL_LDS_BYTES = 60 * 1024;
// rows per workgroup and their LDS stride for dimension d (0, *: no tile)
inline void user_eval_tile(uint32_t d, int& rpb, int& ldp) {
    ldp = (int)(d | 1u);
    const long rows = (long)USER_EVAL_LDS_BYTES / ((long)ldp * 8);
    // (16 rows per workgroup: 4096 rows are 256 workgroups, one per CU, each with 13 16-byte loads per thread in flight -- 64 rows per workgroup left 192
    // CUs idle and took 35 us with a row-by-row copy loop)
    rpb = rows >= 4 ? (int)(rows < 16 ? rows : 16) : 0;
}

// user source + wrapper -> code object for `arch`.  -> "" and `code`, or the reason (compiler log included).  headers: the library's embedded
// files, user_eval.h and user_ln_like.h among them (the latter derives ln_like for a source in the per-coordinate form).
// A source in the PER-DATUM form (it defines BPM_LN_LIKE_DATA: user_eval_data.h) gets that header's kernels instead -- a wavefront per (row, chunk of the data).
// The form is read from the source's own directive: a line `# define BPM_LN_LIKE_DATA <K>` (any blanks or tabs where the preprocessor allows them); the
// name inside a comment or as part of a longer one (BPM_LN_LIKE_DATA_W) is not it.
inline bool user_source_has_data(const std::string& user_src) {
    auto blank = [](char c) { return c == ' ' || c == '\t'; };
    static const std::string def = "define", name = "BPM_LN_LIKE_DATA";
    for (size_t at = 0; at < user_src.size();) {
        size_t eol = user_src.find('\n', at);
        if (eol == std::string::npos) eol = user_src.size();
        size_t i = at;
        while (i < eol && blank(user_src[i])) ++i;
        if (i < eol && user_src[i] == '#') {
            ++i;
            while (i < eol && blank(user_src[i])) ++i;
            if (user_src.compare(i, def.size(), def) == 0 && i + def.size() < eol && blank(user_src[i + def.size()])) {
                i += def.size();
                while (i < eol && blank(user_src[i])) ++i;
                const size_t end = i + name.size();
                if (user_src.compare(i, name.size(), name) == 0 && (end >= eol || blank(user_src[end]) || user_src[end] == '\r')) return true;
            }
        }
        at = eol + 1;
    }
    return false;
}
inline std::string compile_user_likelihood(const std::string& user_src, const std::string& arch, const RtcHeader* headers, size_t n_headers, std::vector<char>& code) {
    const bool data = user_source_has_data(user_src);
    const std::string src = std::string(RTC_PRELUDE) + "#line 1 \"ln_like.hip\"\n" + user_src + (data ? "\n#include \"user_eval_data.h\"\n" : "\n#include \"user_eval.h\"\n");
    return rtc_compile(src, "ln_like.hip", headers, n_headers, arch, {},
                       data ? "the likelihood source does not compile (with data it must define `__device__ void ln_like_datum(const double* x, int d, const double* y, int i, "
                              "const double* p, double* acc)` and `__device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p)`):\n"
                            : "the likelihood source does not compile (it must define `__device__ double ln_like(const double* x, int d, const double* p)`):\n", code);
}

// The per-datum kernels (user_eval_data.h) as the host launches them -- bpm_user_eval_data: rows, ids, n, ld, d, params, data, n_data, n_chunks, out, part;
// bpm_user_fold_data: rows, ids, n, ld, d, params, part, n_data, n_chunks, out; bpm_user_data_info: what the program was compiled with.
using UserEvalDataKernel = void(const double*, const int*, int, int, int, const double*, const double*, int, int, double*, double*);
using UserFoldDataKernel = void(const double*, const int*, int, int, int, const double*, const double*, int, int, double*);
using UserDataInfoKernel = void(int*);
// The chunk of the data a wavefront sums (BPM_DATA_CHUNK of user_eval_data.h; the installed program reports its own and must agree) and the wavefronts of
// a workgroup.  The chunk sums of a batch of rows [row][chunk][K] stay below USER_DATA_SCRATCH_BYTES: more rows go in several launches.
constexpr int USER_DATA_CHUNK = 4096;
constexpr int USER_DATA_WAVES = 4;
constexpr size_t USER_DATA_SCRATCH_BYTES = (size_t)64 << 20;
constexpr int USER_DATA_MAX_W = 64;

// ---- the caller's likelihood INSIDE the update kernel ---------------------------------------------------------------------------------------------
// The second, faster form: the library's own update kernel (kernels.h: phase_fused_kernel, the general instantiation) compiled at run time with the
// caller's function as its target (user_target.h: Target<TARGET_USER>) -- one launch per half generation instead of three.  kernels.h, philox.h and
// the device code of this path travel inside the library as string literals (embedded_src.h, written by the Makefile).  The kernel-argument block
// must be the library's own: the program is compiled with the library's BPM_TEST_HOOKS setting and exports sizeof(PhaseArgs) for the caller to compare.
// Two instantiations: the general one (HOT 0) and the steady-state one (`hot`: 1 with update records, 2 without -- what choose_flavour fixes for
// that flavour is a compile-time constant) -- name_expr[0 / 1]; name_expr[2]: eval_ll_kernel with the same target; name_expr[3]: DREAM's burn-in instantiation (hot + 2).
// `ns`: the inline namespace the program's device code lives in -- unique per module of the process: the library's queue finds kernels by name.
// What is generated here is only what depends on run-time values: the #defines, the explicit instantiations and bpm_user_sizeof.
using UserEvalLlKernel = void(const double*, uint32_t, uint32_t, uint32_t, const double*, double*);      // eval_ll_kernel (kernels.h) as the host launches it from a module
using UserSizeofKernel = void(unsigned int*);                                                             // bpm_user_sizeof, below
inline std::string user_fused_program(const std::string& user_src, const std::string& ns, int algo, int lpc, int dpl, int np, uint32_t dim, bool test_hooks,
                                      int hot, std::vector<std::string>& name_expr) {
    name_expr.assign(4, std::string());
    std::string s;
    s += "typedef unsigned char uint8_t; typedef unsigned short uint16_t; typedef unsigned int uint32_t; typedef unsigned long uint64_t;\n"
         "typedef signed char int8_t; typedef short int16_t; typedef int int32_t; typedef long int64_t;\n";
    s += RTC_PRELUDE;
    s += "#define BPM_VARIANT_NS " + ns + "\n";
    if (test_hooks) s += "#define BPM_TEST_HOOKS 1\n";
    s += "#define BPM_USER_LDP " + std::to_string((int)(dim | 1u)) + "\n";
    s += "#define BPM_USER_DIM " + std::to_string((int)dim) + "\n";      // (the caller's loops over d get a compile-time trip count: the sampler's dimension is fixed)
    s += "#include \"kernels.h\"\n#line 1 \"ln_like.hip\"\n" + user_src + "\n#include \"user_target.h\"\n";
    s += "namespace bpm { inline namespace BPM_VARIANT_NS {\n";
    // [0] general, [1] steady state (HOT 1 / 2), [3] DREAM's burn-in (HOT 3 / 4: sums level 1 of the CR reduction itself, folds the previous generation's sums)
    for (int k = 0; k < 3; ++k) {
        const int h = k == 0 ? 0 : (k == 1 ? hot : hot + 2);
        if (k == 2 && algo != 1 /* ALGO_DREAM */) continue;
        const std::string inst = "phase_fused_kernel<" + std::to_string(algo) + ", TARGET_USER, " + std::to_string(lpc) + ", " + std::to_string(dpl) + ", " +
                                 std::to_string(np) + ", " + std::to_string(h) + ">";
        s += "template __global__ void " + inst + "(const PhaseArgs);\n";
        std::string& e = name_expr[k == 2 ? 3 : k];
        e = "bpm::" + inst;
        e.replace(e.find("TARGET_USER"), 11, "bpm::TARGET_USER");
    }
    // ... and the library's evaluation kernel with the same target: the ln-likes of given states by exactly the arithmetic the update kernel uses
    {
        const std::string inst = "eval_ll_kernel<TARGET_USER, " + std::to_string(lpc) + ", " + std::to_string(dpl) + ">";
        s += "template __global__ void " + inst + "(const double*, uint32_t, uint32_t, uint32_t, const double*, double*);\n";
        name_expr[2] = "bpm::" + inst;
        name_expr[2].replace(name_expr[2].find("TARGET_USER"), 11, "bpm::TARGET_USER");
    }
    s += "extern \"C\" __global__ void bpm_user_sizeof(unsigned int* out) { out[0] = (unsigned int)sizeof(PhaseArgs); out[1] = (unsigned int)block_for(" +
         std::to_string(lpc) + "); out[2] = (unsigned int)block_for_hot(" + std::to_string(lpc) + ", 3, " + std::to_string(dpl) + "); }\n"
         "}}\n";
    return s;
}
// -> "" with `code` and the kernels' lowered (mangled) names, or the reason.  headers: the library's embedded files (kernels.h, philox.h,
// user_target.h and user_ln_like.h among them)
inline std::string compile_user_fused(const std::string& user_src, const std::string& ns, const std::string& arch, const RtcHeader* headers, size_t n_headers,
                                      int algo, int lpc, int dpl, int np, uint32_t dim, bool test_hooks, int hot, std::vector<char>& code, std::string lowered[4]) {
    std::vector<std::string> expr;
    const std::string src = user_fused_program(user_src, ns, algo, lpc, dpl, np, dim, test_hooks, hot, expr);
    return rtc_compile(src, "bpm_user_fused.hip", headers, n_headers, arch, {"-std=c++17", "-Wno-unused-function"},
                       "the update kernel does not compile around this likelihood:\n", code, expr, lowered);
}

}  // namespace BPM_VARIANT_NS
}  // namespace bpm
