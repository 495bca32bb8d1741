// Device and pinned host memory of the sampler library: allocated, owned and freed by the types of this header and by nothing else.
// Included by sampler.hip behind its error plumbing (fail(), HIPCK, CK).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

enum MemKind { MEM_DEVICE, MEM_UNCACHED, MEM_FINEGRAINED, MEM_PINNED };      // hipMalloc | hipExtMallocWithFlags, two flavours | hipHostMalloc
static hipError_t mem_get(void** p, size_t bytes, MemKind k) {
    switch (k) {
        case MEM_UNCACHED: return hipExtMallocWithFlags(p, bytes, hipDeviceMallocUncached);
        case MEM_FINEGRAINED: return hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained);
        case MEM_PINNED: return hipHostMalloc(p, bytes, hipHostMallocDefault);
        default: return hipMalloc(p, bytes);
    }
}
static void mem_put(void* p, MemKind k) {
    if (p) (void)(k == MEM_PINNED ? hipHostFree(p) : hipFree(p));
}
// Memory that lives for one call, or until it is handed to a longer-lived owner: freed on every way out unless leak()ed.  alloc() with a
// `who` first checks the free memory and names the requirement in its error.
template <class T>
struct DevTemp {
    T* p = nullptr;
    MemKind k = MEM_DEVICE;
    DevTemp() = default;
    explicit DevTemp(MemKind k_) : k(k_) {}
    DevTemp(DevTemp&& o) noexcept : p(o.p), k(o.k) { o.p = nullptr; }
    DevTemp& operator=(DevTemp&& o) noexcept {
        if (this != &o) { release(); p = o.p; k = o.k; o.p = nullptr; }
        return *this;
    }
    ~DevTemp() { release(); }
    hipError_t get(size_t n) {      // max(n, 1) elements, the bare HIP error
        release();
        return mem_get(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T), k);
    }
    int alloc(size_t n, const char* who = nullptr, const std::string& what = std::string()) {
        if (who) {
            const size_t need = n * sizeof(T);
            size_t mem_free = 0, mem_total = 0;
            HIPCK(hipMemGetInfo(&mem_free, &mem_total));
            if (need > mem_free)
                return fail(std::string(who) + ": " + what + " need " + std::to_string(need >> 20) + " MiB of device memory; " +
                            std::to_string(mem_free >> 20) + " MiB are free");
        }
        HIPCK(get(n));
        return 0;
    }
    void release() { mem_put(p, k); p = nullptr; }
    T* leak() { T* q = p; p = nullptr; return q; }
};
// What a sampler keeps between calls: every buffer is allocated through its registry, which frees them all -- or forgets them all, where a
// queue that may still run kernels on them could not be stopped (bpm_destroy).  The sampler's members only name the buffers, and pointers INTO
// one (the arena's G, om and control block) are never registered.
struct MemRegistry {
    struct Entry { void* p; MemKind k; };
    std::vector<Entry> all;
    MemRegistry() = default;
    MemRegistry(const MemRegistry&) = delete;
    MemRegistry& operator=(const MemRegistry&) = delete;
    ~MemRegistry() { free_all(); }
    template <class T>
    T* keep(DevTemp<T>& b) {
        all.push_back({b.p, b.k});      // (b owns the buffer until this has succeeded)
        return b.leak();
    }
    template <class T>
    int alloc(T** member, size_t n, MemKind k = MEM_DEVICE) {
        DevTemp<T> b(k);
        CK(b.alloc(n));
        *member = keep(b);
        return 0;
    }
    template <class T>
    void release(T** member) {
        if (!*member) return;
        for (size_t i = 0; i < all.size(); ++i)
            if (all[i].p == static_cast<void*>(*member)) { mem_put(all[i].p, all[i].k); all.erase(all.begin() + (long)i); break; }
        *member = nullptr;
    }
    // `fresh`, filled and waited for, takes the place of *member: the one way a kept buffer grows
    template <class T>
    void replace(T** member, DevTemp<T>& fresh) {
        T* old = *member;
        *member = keep(fresh);
        release(&old);
    }
    void free_all() { for (const Entry& e : all) mem_put(e.p, e.k); all.clear(); }
    void forget_all() { all.clear(); }
};
