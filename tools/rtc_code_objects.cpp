// The code objects of the run-time programs, compiled for gfx950 with no device in the machine: one line per (program, section) with the sha256 of
// .text, .rodata and .note.  Two trees whose lines are equal hand the device the same code for every program below; whole files differ between
// trees in one symbol (__hip_cuid_<hash of the program text>), which is why sections are compared.  A host program around the compile_* wrappers
// of bipymc_amd/csrc (-I chooses the tree; embedded_src.h is written by `make -C bipymc_amd/csrc embedded_src.h`), compiled as plain C++ (-x c++:
// the headers keep their kernels for a HIP compilation, and this program launches none; g++ with the same flags does as well):
//   hipcc -x c++ -O1 -std=c++17 -I bipymc_amd/csrc tools/rtc_code_objects.cpp -o build_variants/rtc_code_objects -ldl && build_variants/rtc_code_objects
// profiles/rtc_code_objects.txt holds its output on a parent commit's tree and on the tree after it.  Reads no file; exit status 1 if a program does not compile.
#include <elf.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#define BPM_VARIANT_NS v_check
#include "derived.h"
#include "pointwise.h"
#include "user_likelihood.h"
#include "embedded_src.h"

namespace {

std::string sha256(const unsigned char* p, size_t n) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74,
        0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d,
        0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e,
        0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5,
        0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::vector<unsigned char> m(p, p + n);
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int k = 7; k >= 0; --k) m.push_back((unsigned char)(((uint64_t)n * 8) >> (8 * k)));
    auto rotr = [](uint32_t x, int r) { return (x >> r) | (x << (32 - r)); };
    for (size_t o = 0; o < m.size(); o += 64) {
        uint32_t w[64], v[8];
        for (int t = 0; t < 16; ++t) w[t] = (uint32_t)m[o + 4 * t] << 24 | (uint32_t)m[o + 4 * t + 1] << 16 | (uint32_t)m[o + 4 * t + 2] << 8 | m[o + 4 * t + 3];
        for (int t = 16; t < 64; ++t)
            w[t] = w[t - 16] + (rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)) + w[t - 7] + (rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10));
        for (int k = 0; k < 8; ++k) v[k] = h[k];
        for (int t = 0; t < 64; ++t) {
            const uint32_t t1 = v[7] + (rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) + K[t] + w[t];
            const uint32_t t2 = (rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
            for (int k = 7; k > 0; --k) v[k] = v[k - 1];
            v[4] += t1;
            v[0] = t1 + t2;
        }
        for (int k = 0; k < 8; ++k) h[k] += v[k];
    }
    char out[65];
    for (int k = 0; k < 8; ++k) snprintf(out + 8 * k, 9, "%08x", h[k]);
    return out;
}

int failures = 0;

// one line per section of the ELF code object `code` (or the reason there is none)
void report(const char* name, const std::string& why, const std::vector<char>& code) {
    if (!why.empty()) { printf("# %s does not compile: %s\n", name, why.c_str()); ++failures; return; }
    const unsigned char* b = reinterpret_cast<const unsigned char*>(code.data());
    const Elf64_Ehdr* eh = reinterpret_cast<const Elf64_Ehdr*>(b);
    if (code.size() < sizeof(Elf64_Ehdr) || std::string(code.data(), 4) != ELFMAG || eh->e_shoff + (uint64_t)eh->e_shnum * sizeof(Elf64_Shdr) > code.size()) {
        printf("# %s: not an ELF code object\n", name); ++failures; return;
    }
    const Elf64_Shdr* sh = reinterpret_cast<const Elf64_Shdr*>(b + eh->e_shoff);
    const char* names = code.data() + sh[eh->e_shstrndx].sh_offset;
    for (const char* want : {".text", ".rodata", ".note"}) {
        std::string sum = "(no such section)";
        for (int k = 0; k < eh->e_shnum; ++k)
            if (std::string(names + sh[k].sh_name) == want && sh[k].sh_offset + sh[k].sh_size <= code.size()) sum = sha256(b + sh[k].sh_offset, sh[k].sh_size);
        printf("%s  %s %s\n", sum.c_str(), name, want);
    }
}

const size_t N_HDR = sizeof(bpm_embedded) / sizeof(bpm_embedded[0]);
const char* ARCH = "gfx950";

// a diagonal Gaussian in the plain, the per-coordinate and the per-datum form (examples/ex_hip_likelihood.py, ex_data_likelihood.py in small)
const char* LIKE_PLAIN =
    "__device__ double ln_like(const double* x, int d, const double* p) {\n"
    "    double s = 0.0;\n    for (int j = 0; j < d; ++j) { const double z = (x[j] - p[j]) / p[d + j]; s += z * z; }\n    return -0.5 * s;\n}";
const char* LIKE_TERMS =
    "#define BPM_LN_LIKE_TERMS 1\n"
    "__device__ void ln_like_terms(double xj, int j, int d, const double* p, double* acc) { const double z = (xj - p[j]) / p[d + j]; acc[0] += z * z; }\n"
    "__device__ double ln_like_finish(const double* acc, int d, const double* p) { return -0.5 * acc[0]; }";
const char* LIKE_DATA =
    "#define BPM_LN_LIKE_DATA 1\n#define BPM_LN_LIKE_DATA_W 2\n"
    "__device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc) {\n"
    "    const double r = y[1] - (x[0] + x[1] * y[0]); acc[0] += r * r; }\n"
    "__device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p) { return -0.5 * acc[0] * p[0]; }";
const char* DERIVE =
    "__device__ void derive(const double* x, int d, double ll, const double* p, double* out) { out[0] = x[2] / x[1]; out[1] = x[0] + x[1] * p[0] + ll; }";
// the straight-line fit of tests/_waic_cases.py: SOURCES[1] for w = 1; for w > 1 SOURCES[3] and [9] with every value of the datum read, the
// last one where those read it and the ones between in a sum (a value that is not read is not loaded: the probe would not hold w values)
#define POINT_HEAD "__device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p) {\n"
std::string point_source(int w) {
    if (w == 1) return POINT_HEAD "    const double r = y[0] - x[0];\n    return -0.5 * r * r * p[0] + x[d - 1] * p[1] - i * p[2];\n}";
    return POINT_HEAD "    const double r = y[1] - (x[0] + x[1] * y[0]);\n    double t = 0.0;\n    for (int k = 2; k < " + std::to_string(w - 1) +
           "; ++k) t += y[k];\n    return -0.5 * r * r * p[0] + x[d - 1] * y[" + std::to_string(w - 1) + "] - i * p[2] + t * p[1];\n}";
}

}  // namespace

int main() {
    std::vector<char> code;
    const struct { const char* name; const char* src; } likes[] = {{"eval_plain", LIKE_PLAIN}, {"eval_terms", LIKE_TERMS}, {"eval_data", LIKE_DATA}};
    for (const auto& l : likes) report(l.name, bpm::compile_user_likelihood(l.src, ARCH, bpm_embedded, N_HDR, code), code);
    // the update kernel around the likelihood: (algo, lpc, dpl, np, dim, hot) of three kernel shapes (algo 1: DREAM, 0: DE-MC), both forms
    const struct { const char* name; int algo, lpc, dpl, np, dim, hot; } shapes[] = {
        {"fused_dream_lpc64_dim100", 1, 64, 2, 3, 100, 1}, {"fused_dream_lpc4_dim8", 1, 4, 2, 3, 8, 1}, {"fused_demc_lpc1_dim2", 0, 1, 2, 1, 2, 2}};
    for (const auto& s : shapes)
        for (int terms = 0; terms < 2; ++terms) {
            std::string lowered[4];
            const std::string name = std::string(s.name) + (terms ? "_terms" : "_plain");
            report(name.c_str(), bpm::compile_user_fused(terms ? LIKE_TERMS : LIKE_PLAIN, "v_check", ARCH, bpm_embedded, N_HDR, s.algo, s.lpc, s.dpl, s.np, (uint32_t)s.dim,
                                                         false, s.hot, code, lowered), code);
        }
    report("derive", bpm::compile_device_function(DERIVE, ARCH, bpm_embedded, N_HDR, code), code);
    // w below, at and above the cut-off of a datum's values in registers, and the largest
    for (const int w : {1, 8, 9, 64}) {
        const std::string n = std::to_string(w), src = point_source(w);
        report(("pointwise_w" + n).c_str(), bpm::compile_pointwise(src, w, ARCH, bpm_embedded, N_HDR, code), code);
        report(("pointwise_tail_w" + n).c_str(), bpm::compile_pointwise_tail(src, w, ARCH, bpm_embedded, N_HDR, code), code);
    }
    return failures ? 1 : 0;
}
