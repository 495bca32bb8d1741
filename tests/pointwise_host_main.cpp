// Stand-alone host program of tests/test_waic_host.py: the launch layout of bipymc_amd/csrc/pointwise.h and the log-sum-exp merge of
// pointwise_rows.h, compiled without a device and run under the address and undefined-behaviour sanitizers.  Prints counts, one per line.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I bipymc_amd/csrc tests/pointwise_host_main.cpp -o pointwise_host -ldl
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#define BPM_VARIANT_NS host_check
#include "pointwise.h"

namespace {

// what the kernel and the host rely on for a layout of n_rows rows of d coordinates over n_data data
bool layout_ok(uint32_t d, uint64_t n_rows, uint64_t n_data) {
    const bpm::PointwiseLayout L = bpm::pointwise_layout(d, n_rows, n_data);
    bool ok = L.n_tiles * bpm::PW_THREADS >= n_data && (L.n_tiles - 1) * bpm::PW_THREADS < n_data;
    ok = ok && L.R >= 1 && L.R <= bpm::PW_THREADS && (L.ldp == 0 ? L.R == bpm::PW_THREADS : (L.ldp == (d | 1u) && L.R >= bpm::PW_MIN_TILE_ROWS));
    ok = ok && (uint64_t)L.R * L.ldp * 8u <= L.lds_bytes && L.lds_bytes <= bpm::PW_LDS_BYTES && L.lds_bytes % 16u == 0;
    ok = ok && L.parts >= 1 && L.chunk >= 1 && L.chunk < (1ull << 31) && L.parts * L.chunk >= n_rows && (L.parts - 1) * L.chunk < n_rows;
    const uint64_t aimed = bpm::PW_GRID / L.n_tiles > 1 ? bpm::PW_GRID / L.n_tiles : 1, fewest = (n_rows >> 31) + 1;
    ok = ok && L.parts <= (aimed > fewest ? aimed : fewest);
    // the parts as the kernel cuts them: inside the window, none empty, the last one ends the window (all of them where they are few)
    uint64_t seen = 0;
    const bool all = L.parts <= 4096;
    const uint64_t some[] = {0, 1, L.parts / 2, L.parts - 2, L.parts - 1};
    for (uint64_t k = 0; k < (all ? L.parts : 5); ++k) {
        const uint64_t p = all ? k : some[k];
        if (p >= L.parts) continue;
        uint64_t r0 = p * L.chunk;
        r0 = r0 < n_rows ? r0 : n_rows;
        const uint64_t r1 = r0 + L.chunk < n_rows ? r0 + L.chunk : n_rows;
        ok = ok && r1 > r0 && r1 - r0 <= L.chunk && (p != L.parts - 1 || r1 == n_rows);
        seen += r1 - r0;
    }
    if (all) ok = ok && seen == n_rows;
    if (!ok) std::printf("# layout: d=%u n_rows=%llu n_data=%llu -> R=%u ldp=%u lds=%u tiles=%llu parts=%llu chunk=%llu\n", d, (unsigned long long)n_rows,
                         (unsigned long long)n_data, L.R, L.ldp, L.lds_bytes, (unsigned long long)L.n_tiles, (unsigned long long)L.parts, (unsigned long long)L.chunk);
    return ok;
}

struct Lse { unsigned long long n; double m, s; };

Lse of(const std::vector<double>& v) {
    Lse a{0, -std::numeric_limits<double>::infinity(), 0.0};
    for (double l : v) {      // the kernel's online update
        if (a.n == 0) { a.m = l; a.s = 1.0; }
        else if (l > a.m) { a.s = a.s * std::exp(a.m - l) + 1.0; a.m = l; }
        else a.s += std::exp(l - a.m);
        ++a.n;
    }
    return a;
}

long double exact(const std::vector<double>& v) {
    long double top = -std::numeric_limits<long double>::infinity(), tot = 0.0L;
    for (double l : v) top = l > top ? l : top;
    for (double l : v) tot += std::exp((long double)l - top);
    return top + std::log(tot);
}

}   // namespace

int main() {
    long long layouts = 0, layout_bad = 0, merges = 0, merge_bad = 0;
    const uint32_t ds[] = {1, 2, 3, 63, 100, 127, 128, 129, 479, 640, 2047, 100000};
    const uint64_t rows[] = {1, 2, 15, 16, 17, 63, 64, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 2050, 65536, 1000003, 2457600, (1ull << 31) - 1, 1ull << 31,
                             (1ull << 31) + 1, 6000000000ull, (1ull << 40) + 7};
    const uint64_t data[] = {1, 63, 64, 65, 255, 256, 257, 529, 1000, 10000, 100000, 524288, 524289, (1ull << 31) - 1};
    for (uint32_t d : ds)
        for (uint64_t r : rows)
            for (uint64_t nd : data) { ++layouts; layout_bad += !layout_ok(d, r, nd); }
    for (uint64_t r = 1; r < 12000; r += 1) { ++layouts; layout_bad += !layout_ok(3, r, 200); }

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<std::vector<double>> sides = {{}, {0.0}, {-745.5}, {1e300}, {-1e300, -1e300}, {3.0, 1.0, 2.0}, {-1700.0, -100.0, -900.0}, {709.0, 708.5},
                                                    {-0.25, -0.25, -0.25, -0.25}, {5e-324, 0.0, -5e-324}};
    for (const auto& a : sides)
        for (const auto& b : sides)
            for (double junk : {nan, inf, -inf}) {      // what an empty side holds is never read
                Lse x = of(a), y = of(b);
                if (a.empty()) { x.m = junk; x.s = junk; }
                if (b.empty()) { y.m = junk; y.s = junk; }
                pw_merge_lse(x.n, x.m, x.s, y.n, y.m, y.s);
                ++merges;
                std::vector<double> all(a);
                all.insert(all.end(), b.begin(), b.end());
                bool ok = true;
                if (all.empty()) ok = a.empty() && b.empty();      // (nothing to say: the caller reads neither m nor s)
                else {
                    const long double got = (long double)x.m + std::log((long double)x.s), want = exact(all);
                    ok = x.s == x.s && x.m == x.m && x.s >= 1.0 && std::fabs(got - want) <= 64 * 0x1p-53L * (1.0L + std::fabs(want));
                }
                if (!ok) std::printf("# merge: sides of %zu and %zu values give m=%a s=%a\n", a.size(), b.size(), x.m, x.s);
                merge_bad += !ok;
            }
    const bpm::PointwiseLayout L = bpm::pointwise_layout(3, 2050, 200);
    std::printf("layouts %lld\nlayout_violations %lld\nmerges %lld\nmerge_violations %lld\n", layouts, layout_bad, merges, merge_bad);
    std::printf("layout_3_2050_200 %u %u %llu %llu\n", bpm::PW_THREADS, L.R, (unsigned long long)L.parts, (unsigned long long)L.chunk);
    return 0;
}
