// WAIC's ingredients per datum, reduced where the history lives: the host side of pointwise_rows.h (which states the kernel, its order of
// operations and the record).  The reference has no such statistic; its fitting scripts sum a log density over their data points inside
// ln_like_fn (examples/ex_line_fit.py:63-67) -- here the caller writes ONE term of that sum,
//     __device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p)
// and the library compiles bpm_pointwise_rows around it (hiprtc through rtc.h's one compile path, -O3 -ffp-contract=off).  This file holds the
// compile wrapper, the launch layout -- a function of (n_rows, n_data, d) alone, which is what makes the result's bits a function of (window,
// data, params) -- the kernel's parameter list as the host launches it, and the library's own fold kernel over the parts.
// Everything above the fold kernel is plain C++: tests/pointwise_host_main.cpp compiles it without a device.
#pragma once
#include "pointwise_rows.h"      // (BPM_POINTWISE_W undefined: the record's fields and pw_merge_lse only)
#include "user_likelihood.h"

namespace bpm {
inline namespace BPM_VARIANT_NS {

constexpr uint32_t PW_THREADS = 256;             // T: data per tile, threads per workgroup
constexpr uint32_t PW_LDS_BYTES = 16 * 1024;     // a workgroup's row tile: small, so that LDS never bounds the residency (the kernel is bound by exp, not by memory)
constexpr uint32_t PW_MIN_TILE_ROWS = 16;        // fewer rows than this per tile: rows are read where they lie
constexpr uint32_t PW_GRID = 2048;               // workgroups aimed at: the device a few times over
constexpr int PW_MAX_W = USER_DATA_MAX_W;

// bpm_pointwise_rows as the host launches it: H, ld, d, lo, hi, chunk, n_tiles, params, data, n_data, R, ldp, rec, n_rec, values
using PointwiseRowsKernel = void(const double*, unsigned int, int, unsigned long long, unsigned long long, unsigned long long, unsigned int, const double*,
                                 const double*, unsigned int, unsigned int, unsigned int, double*, unsigned long long, double*);

struct PointwiseLayout {
    uint32_t R = 0, ldp = 0, lds_bytes = 0;      // rows per tile, their LDS stride (0: not staged), the dynamic LDS
    uint64_t n_tiles = 0, parts = 0, chunk = 0;  // data tiles, row parts, rows per part (the last part: what is left)
};

// The launch of n_rows rows of d coordinates over n_data data.  Tile: R = min(256, PW_LDS_BYTES / 8 / (d | 1)) rows, none (R = 256 rows per
// sweep, read in place) below 16.  Parts: PW_GRID / n_tiles of them (at least 1), but none shorter than 4 tiles and none of 2^31 rows or
// more (a thread's uint32 counts); then chunk = ceil(n_rows / parts) and parts = ceil(n_rows / chunk): no part is empty.
inline PointwiseLayout pointwise_layout(uint32_t d, uint64_t n_rows, uint64_t n_data) {
    PointwiseLayout L;
    L.ldp = d | 1u;
    const uint32_t rows = PW_LDS_BYTES / 8u / L.ldp;
    if (rows < PW_MIN_TILE_ROWS) { L.ldp = 0u; L.R = PW_THREADS; }
    else L.R = rows < PW_THREADS ? rows : PW_THREADS;
    L.lds_bytes = (L.R * L.ldp * 8u + 15u) & ~15u;
    L.n_tiles = (n_data + PW_THREADS - 1) / PW_THREADS;
    if (n_rows == 0 || n_data == 0) return L;
    uint64_t parts = PW_GRID / L.n_tiles > 1 ? PW_GRID / L.n_tiles : 1;
    const uint64_t longest = (n_rows + 4ull * L.R - 1) / (4ull * L.R);
    parts = parts < longest ? parts : longest;
    const uint64_t fewest = (n_rows >> 31) + 1;
    parts = parts > fewest ? parts : fewest;
    L.chunk = (n_rows + parts - 1) / parts;
    L.parts = (n_rows + L.chunk - 1) / L.chunk;
    return L;
}

// caller's source + wrapper -> code object for `arch`.  -> "" and `code`, or the reason (compiler log included)
inline std::string compile_pointwise(const std::string& user_src, int w, const std::string& arch, const RtcHeader* headers, size_t n_headers, std::vector<char>& code) {
    const std::string src = std::string(RTC_PRELUDE) + "#define BPM_POINTWISE_W " + std::to_string(w) + "\n#line 1 \"ln_like_point.hip\"\n" + user_src +
                            "\n#include \"pointwise_rows.h\"\n";
    return rtc_compile(src, "ln_like_point.hip", headers, n_headers, arch, {},
                       "the pointwise source does not compile (it must define `__device__ double ln_like_point(const double* x, int d, const double* y, int i, "
                       "const double* p)`):\n", code);
}

// ---- PSIS-LOO's streaming stages (pointwise_tail.h states the kernels; psis.h fits and finishes) ------------------------------------------
constexpr uint32_t PT_HIST_BYTES = 16 * 1024;    // the radix select's 16 counters per lane, behind the row tile in LDS

// bpm_pointwise_tail: H, ld, d, lo, hi, chunk, n_tiles, tile0, params, data, n_data, R, ldp, lds_rows, keep, cap, buf, cnt, bad, compactions
using PointwiseTailKernel = void(const double*, unsigned int, int, unsigned long long, unsigned long long, unsigned long long, unsigned int, unsigned int,
                                 const double*, const double*, unsigned int, unsigned int, unsigned int, unsigned int, const unsigned int*, unsigned int,
                                 unsigned long long*, unsigned int*, unsigned int*, unsigned int*);
// bpm_pointwise_tail_final: n_tiles, tile0, parts, n_data, keep, cap, k_max, buf, cnt, bad, out, n_kept, n_bad
using PointwiseTailFinalKernel = void(unsigned int, unsigned int, unsigned int, unsigned int, const unsigned int*, unsigned int, unsigned int, unsigned long long*,
                                      const unsigned int*, const unsigned int*, unsigned long long*, unsigned int*, unsigned int*);
// bpm_pointwise_body: H, ld, d, lo, hi, chunk, n_tiles, tile0, params, data, n_data, R, ldp, cut, rec, n_rec
using PointwiseBodyKernel = void(const double*, unsigned int, int, unsigned long long, unsigned long long, unsigned long long, unsigned int, unsigned int,
                                 const double*, const double*, unsigned int, unsigned int, unsigned int, const double*, double*, unsigned long long);

// Stage A's launch: the data go in batches of `batch_tiles` tiles; a batch's rows in `parts` parts of `chunk` rows, each (tile, part) with a
// candidate buffer of 256 columns of cap = 2 k_max keys.  Unlike pointwise_layout this one may depend on the scratch budget: selection is exact.
struct LooLayout {
    uint64_t batch_tiles = 0, batches = 0, parts = 0, chunk = 0, cap = 0;
    uint64_t per_tile_bytes = 0;      // of one tile of a batch: its parts' buffers and counters, the final keys twice (the sort's in and out), the fit's work space, stage B's records
    bool fits = false;
    bool too_many_keys = false;       // one tile's final keys (256 k_max) are beyond the sort's 32-bit index: no budget helps
};

// Parts: as many as keep the device busy (PW_GRID / batch_tiles), none shorter than max(4 R, 8 k_max) rows -- a part must be long against its
// buffer for the threshold to do its work -- none of 2^31 rows or more, and no more than the budget holds.  fits = false: not even one tile
// with one part fits (per_tile_bytes says what that takes, the sort's temporaries not counted).
inline LooLayout loo_layout(const PointwiseLayout& P, uint64_t n_rows, uint64_t k_max, uint64_t work_doubles, uint64_t budget) {
    LooLayout L;
    L.cap = 2 * k_max;
    if (n_rows == 0 || P.n_tiles == 0 || k_max == 0) return L;
    const uint64_t T = PW_THREADS;
    const uint64_t part_bytes = T * L.cap * 8 + T * 8 + 4;                                      // buffer | cnt, bad | compactions
    const uint64_t tile_fixed = 2 * T * k_max * 8 + T * 8 + T * work_doubles * 8 + T * 8 + 3 * P.parts * T * 8;      // keys in, out | n_kept, n_bad | work | cut | body records
    const uint64_t shortest = 4ull * P.R > 8 * k_max ? 4ull * P.R : 8 * k_max;
    uint64_t by_rows = n_rows / shortest > 1 ? n_rows / shortest : 1;
    const uint64_t fewest = (n_rows >> 31) + 1;
    by_rows = by_rows > fewest ? by_rows : fewest;
    L.per_tile_bytes = fewest * part_bytes + tile_fixed;
    if (L.per_tile_bytes > budget) return L;
    L.fits = true;
    uint64_t bt = budget / L.per_tile_bytes;
    bt = bt < P.n_tiles ? bt : P.n_tiles;
    const uint64_t most_keys = ((1ull << 31) - 1) / (T * k_max);      // (the segmented sort indexes a batch's keys with 32 bits)
    bt = bt < most_keys ? bt : most_keys;
    if (bt == 0) { L.fits = false; L.too_many_keys = true; return L; }
    uint64_t parts = PW_GRID / bt > 1 ? PW_GRID / bt : 1;
    parts = parts < by_rows ? parts : by_rows;
    const uint64_t by_budget = (budget / bt - tile_fixed) / part_bytes;
    parts = parts < by_budget ? parts : by_budget;
    parts = parts > fewest ? parts : fewest;
    L.chunk = (n_rows + parts - 1) / parts;
    L.parts = (n_rows + L.chunk - 1) / L.chunk;
    L.batch_tiles = bt;
    L.batches = (P.n_tiles + bt - 1) / bt;
    L.per_tile_bytes = L.parts * part_bytes + tile_fixed;
    return L;
}

// caller's source + pointwise_tail.h -> code object for `arch` (the kernels of stages A and B).  -> "" and `code`, or the reason
inline std::string compile_pointwise_tail(const std::string& user_src, int w, const std::string& arch, const RtcHeader* headers, size_t n_headers, std::vector<char>& code) {
    const std::string src = std::string(RTC_PRELUDE) + "#define BPM_POINTWISE_W " + std::to_string(w) + "\n#line 1 \"ln_like_point.hip\"\n" + user_src +
                            "\n#include \"pointwise_tail.h\"\n";
    return rtc_compile(src, "ln_like_point.hip", headers, n_headers, arch, {},
                       "the pointwise source does not compile (it must define `__device__ double ln_like_point(const double* x, int d, const double* y, int i, "
                       "const double* p)`):\n", code);
}

#if defined(__HIPCC__)
// The parts of every datum in index order -> one folded record per datum (pointwise_rows.h, step 4).  part: PW_FIELDS fields of parts * n_data
// records; out: PW_FIELDS fields of n_data records.
__global__ __launch_bounds__(PW_THREADS) void pw_fold_kernel(const double* __restrict__ part, uint32_t parts, uint64_t n_data, double* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * PW_THREADS + threadIdx.x;
    if (j >= n_data) return;
    const uint64_t n_rec = n_data * parts;
    const unsigned long long* pu = reinterpret_cast<const unsigned long long*>(part);
    unsigned long long* ou = reinterpret_cast<unsigned long long*>(out);
    unsigned long long n = 0ull, n_nan = 0ull, n_pinf = 0ull, n_ninf = 0ull;
    double c = 0.0, s1 = 0.0, s2 = 0.0, m = -__longlong_as_double(0x7FF0000000000000ll), s = 0.0;
    for (uint32_t p = 0; p < parts; ++p) {
        const uint64_t q = (uint64_t)p * n_data + j;
        const unsigned long long nb = pu[PW_N * n_rec + q];
        pw_merge_lse(n, m, s, nb, part[PW_M * n_rec + q], part[PW_S * n_rec + q]);      // (before the moments' merge moves n)
        tr_merge_moments(n, c, s1, s2, nb, part[PW_C * n_rec + q], part[PW_S1 * n_rec + q], part[PW_S2 * n_rec + q]);
        n_nan += pu[PW_NAN * n_rec + q];
        n_pinf += pu[PW_PINF * n_rec + q];
        n_ninf += pu[PW_NINF * n_rec + q];
    }
    ou[PW_N * n_data + j] = n;
    out[PW_C * n_data + j] = c;
    out[PW_S1 * n_data + j] = s1;
    out[PW_S2 * n_data + j] = s2;
    ou[PW_NAN * n_data + j] = n_nan;
    ou[PW_PINF * n_data + j] = n_pinf;
    ou[PW_NINF * n_data + j] = n_ninf;
    out[PW_M * n_data + j] = m;
    out[PW_S * n_data + j] = s;
}
#endif

}  // namespace BPM_VARIANT_NS
}  // namespace bpm
