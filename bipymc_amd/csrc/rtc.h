// Run-time compilation with hiprtc: the ONE place that creates a program, compiles it, fetches its log, its code and its lowered names
// (user_likelihood.h and derived.h assemble the program texts).  hiprtc is loaded on demand (libhiprtc.so): a process that never installs a
// likelihood or a function given as source never needs it.
#pragma once
#include <dlfcn.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace bpm {
inline namespace BPM_VARIANT_NS {

struct Hiprtc {
    void* lib = nullptr;
    int (*CreateProgram)(void**, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
    int (*CompileProgram)(void*, int, const char* const*) = nullptr;
    int (*GetProgramLogSize)(void*, size_t*) = nullptr;
    int (*GetProgramLog)(void*, char*) = nullptr;
    int (*GetCodeSize)(void*, size_t*) = nullptr;
    int (*GetCode)(void*, char*) = nullptr;
    int (*DestroyProgram)(void**) = nullptr;
    int (*AddNameExpression)(void*, const char*) = nullptr;
    int (*GetLoweredName)(void*, const char*, const char**) = nullptr;
};

// -> "" or the reason hiprtc cannot be used
inline std::string load_hiprtc(Hiprtc& h) {
    if (h.lib) return "";
    const char* names[] = {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
    void* lib = nullptr;
    for (const char* n : names) {
        lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (lib) break;
    }
    if (!lib) return std::string("cannot load hiprtc: ") + dlerror();
#define BPM_RTC_SYM(f)                                                              \
    h.f = reinterpret_cast<decltype(h.f)>(dlsym(lib, "hiprtc" #f));                 \
    if (!h.f) return "hiprtc symbol hiprtc" #f " missing";
    BPM_RTC_SYM(CreateProgram) BPM_RTC_SYM(CompileProgram) BPM_RTC_SYM(GetProgramLogSize) BPM_RTC_SYM(GetProgramLog)
    BPM_RTC_SYM(GetCodeSize) BPM_RTC_SYM(GetCode) BPM_RTC_SYM(DestroyProgram) BPM_RTC_SYM(AddNameExpression) BPM_RTC_SYM(GetLoweredName)
#undef BPM_RTC_SYM
    h.lib = lib;
    return "";
}

// What a caller's source may use without an include (hiprtc declares the device math functions -- exp, log, sqrt, lgamma, erf ... -- but not
// <cmath>'s macros: a prior returns -INFINITY)
constexpr const char* RTC_PRELUDE =
    "#ifndef INFINITY\n#define INFINITY (__builtin_huge_val())\n#endif\n"
    "#ifndef NAN\n#define NAN (__builtin_nan(\"\"))\n#endif\n"
    "#ifndef M_PI\n#define M_PI 3.14159265358979323846\n#endif\n";

// A file the program text may #include: the library's own headers travel inside it as string literals (embedded_src.h, written by the Makefile)
struct RtcHeader {
    const char* name;
    const char* text;
};

// Program text `src` (called `name` in the compiler's messages) -> code object for `arch` ("gfx950", or a device's gcnArchName), compiled with
// -O3 -ffp-contract=off (f64 arithmetic unfused, like the library's own kernels: a formula written the same way in NumPy gives the same bits)
// and `extra_opts`.  exprs: name expressions to lower (an empty one is skipped), lowered: their mangled names, index by index.
// -> "" with `code` (and `lowered`), or the reason: `not_compiling` + the compiler's log when the text does not compile.
// One compilation at a time per process: the mutex covers the loader's state and hiprtc's own.
inline std::string rtc_compile(const std::string& src, const char* name, const RtcHeader* headers, size_t n_headers, const std::string& arch,
                               const std::vector<const char*>& extra_opts, const std::string& not_compiling, std::vector<char>& code,
                               const std::vector<std::string>& exprs = {}, std::string* lowered = nullptr) {
    static Hiprtc h;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    const std::string why = load_hiprtc(h);
    if (!why.empty()) return why;
    std::vector<const char*> hdr_src, hdr_names;
    for (size_t i = 0; i < n_headers; ++i) { hdr_src.push_back(headers[i].text); hdr_names.push_back(headers[i].name); }
    struct Program {      // destroyed on every way out
        Hiprtc& h;
        void* p = nullptr;
        ~Program() { if (p) h.DestroyProgram(&p); }
    } prog{h};
    if (h.CreateProgram(&prog.p, src.c_str(), name, (int)n_headers, hdr_src.data(), hdr_names.data()) != 0 || !prog.p) return "hiprtcCreateProgram failed";
    for (const std::string& e : exprs)
        if (!e.empty() && h.AddNameExpression(prog.p, e.c_str()) != 0) return "hiprtcAddNameExpression failed";
    const std::string a = "--offload-arch=" + arch;
    std::vector<const char*> opts = {a.c_str(), "-O3", "-ffp-contract=off"};
    opts.insert(opts.end(), extra_opts.begin(), extra_opts.end());
    const int rc = h.CompileProgram(prog.p, (int)opts.size(), opts.data());
    std::string log;
    size_t n = 0;
    if (h.GetProgramLogSize(prog.p, &n) == 0 && n > 1) {
        log.resize(n);
        if (h.GetProgramLog(prog.p, &log[0]) != 0) log.clear();
        while (!log.empty() && (log.back() == '\0' || log.back() == '\n')) log.pop_back();
    }
    if (rc != 0) return not_compiling + log;
    for (size_t k = 0; k < exprs.size(); ++k) {
        const char* low = nullptr;
        if (exprs[k].empty()) { lowered[k].clear(); continue; }
        if (h.GetLoweredName(prog.p, exprs[k].c_str(), &low) != 0 || !low) return "hiprtcGetLoweredName failed for " + exprs[k];
        lowered[k] = low;
    }
    size_t sz = 0;
    if (h.GetCodeSize(prog.p, &sz) != 0 || sz == 0) return "hiprtcGetCodeSize failed";
    code.resize(sz);
    if (h.GetCode(prog.p, code.data()) != 0) return "hiprtcGetCode failed";
    return "";
}

// `text` into a caller's buffer of `cap` bytes, cut to fit and always terminated (no buffer: nothing)
inline void copy_text(const std::string& text, char* buf, int64_t cap) {
    if (!buf || cap <= 0) return;
    const size_t n = std::min(text.size(), (size_t)cap - 1);
    std::memcpy(buf, text.data(), n);
    buf[n] = '\0';
}

}  // namespace BPM_VARIANT_NS
}  // namespace bpm
