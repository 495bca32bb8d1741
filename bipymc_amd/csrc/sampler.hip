// Host side of libbipymc_hip.so: the sampler object behind the C ABI of
// include/bipymc_hip.h.  It owns the device state (replicated chain-state matrix,
// log-like cache, history, Welford moments, CR statistics) and runs the generation
// loop of bipymc/demc.py:63-151 as back-to-back dispatches on a user-mode AQL queue of
// the library's own (aql_queue.h) or on one HIP stream.  For world_size > 1 the two
// MPI_Allgathers per generation (demc.py:93-94,116-117) are replaced by the PUSH
// exchange -- the owner of a chain stores an accepted row into every other rank's
// replica from inside the update kernel (IPC-mapped buffers), a one-wavefront kernel
// orders the ranks -- or, as the fallback, by in-place RCCL all-gathers on the stream:
// of one accept byte per chain followed by a replay of the accepted proposals, of
// packed accepted rows, or of whole rank blocks.
#include <dlfcn.h>
#include <sys/mman.h>
#include <unistd.h>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstddef>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/bipymc_hip.h"
#include "kernels.h"
#include "kernels_wide.h"
#include "diagnostics.h"
#include "quantiles.h"
#include "covariance.h"
#include "histograms.h"
#include "traces.h"
#include "ranks.h"
// bpm_rank_history's sort: rocPRIM's segmented radix sort (header-only).  Its kernels go into this variant's own inline namespace, like the
// library's own (philox.h: BPM_VARIANT_NS) -- two variants in one process must not share a kernel symbol.  (After <cstring>, which one of
// its headers needs.)
#define ROCPRIM_INLINE_NAMESPACE BPM_VARIANT_NS
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#ifdef BPM_TEST_HOOKS
#include "rocrand_check.h"
#include "accept_check.h"
#endif
#include "aql_queue.h"
#include "user_likelihood.h"
#include "derived.h"
#include "pointwise.h"
#include "psis.h"
#include "embedded_src.h"

using namespace bpm;

// The host code below launches the update kernels the way the preload build compiles them (leading arguments in SGPRs, the specialised
// instantiations): every target of csrc/Makefile defines it.  (kernels.h keeps its own #ifdef: hiprtc compiles it WITHOUT, user_likelihood.h.)
#ifndef BPM_PRELOAD
#error "sampler.hip needs -DBPM_PRELOAD -mllvm -amdgpu-kernarg-preload-count=5 (the flag pair of CXXFLAGS in csrc/Makefile)"
#endif

// The ONE environment variable that changes which kernels / launch shapes the library uses: BPM_TEST_PATHS, a comma-separated list read
// once per process, for the tests that pin every alternative kernel path to the default one bit for bit
// (tests/test_gpu_api.py::test_alternative_kernel_paths_on_one_gpu) and for the timing tools:
//   mode1        one work item per LOCAL chain filtered by its position (what a rank of a world without sorted records launches)
//   noplan       header block and partner ids drawn in the update kernel (what > 16384 chains per GPU use) instead of plan records
//   noperm       the shuffle bijection walked in the kernel instead of looked up
//   planall      plan records whatever the number of chains
//   nohot        the general kernel instantiation instead of the specialised ones
//   groupqueues  every rank of a local group on an AQL queue of its own (the ranks' barrier kernels wait for each other across queues)
//   wt8          rows written through with two 8-byte agent-scope atomic stores per lane (round 2's form) instead of one 16-byte sc1 store
//   ctrlarena    the push exchange's control block inside the coarse-grained arena instead of a fine-grained allocation of its own
//   serial       the emulated ranks of a local group take turns on the GPU (tools/emulate_ranks.py)
//   hosttiming   host nanoseconds spent preparing generations and inside launch calls, printed by bpm_destroy
// Operational switches (documented in README.md): BPM_DIRECT_QUEUE=0, BPM_QUEUE_INFLIGHT, BPM_QUEUE_TIMEOUT_S, BPM_EXCHANGE, BPM_VERBOSE.
// The PRODUCT library does not read it: BPM_TEST_PATHS, the bpm_debug_* / bpm_selftest_* entry points and the BPM_FAKE_* timing builds exist
// only in build_variants/libbipymc_test.so (-DBPM_TEST_HOOKS, declared in include/bipymc_hip_test.h); the GPU tests that need them load
// that variant, the parity tests run against the product library.
#ifdef BPM_TEST_HOOKS
static bool test_path(const char* name) {
    static const std::string all = [] { const char* e = getenv("BPM_TEST_PATHS"); return std::string(",") + (e ? e : "") + ","; }();
    return all.find(std::string(",") + name + ",") != std::string::npos;
}
#else
static constexpr bool test_path(const char*) { return false; }
#endif

static thread_local std::string g_err;
static int fail(const std::string& m) {
    g_err = m;
    return 1;
}
#define HIPCK(expr)                                                                                    \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" + __FILE__ + ":" + \
                        std::to_string(__LINE__) + ")");                                               \
    } while (0)
#define CK(expr)                 \
    do {                         \
        int _r = (expr);         \
        if (_r != 0) return _r;  \
    } while (0)

// Wait for a stream by POLLING it (up to spin_ms, then a blocking wait).  hipStreamSynchronize parks the calling thread; on
// this class of host the core then drops to its base clock and the launch calls that follow take ~4.7 us instead of ~2.4 us
// for the first few hundred microseconds -- longer than the 6 us the GPU needs per update kernel, so a short bpm_step call
// issued right after a wait ran HOST-paced (profiles/r02_host_launch_pacing.txt).  A polling wait keeps the core clocked up.
// (50 ms of polling cover the short calls this is for -- a 1000-generation step is 11 ms; longer waits park the thread instead of burning a
// core per rank: ADVICE r02)
static int wait_stream(hipStream_t st, double spin_ms = 50.0) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) { (void)hipGetLastError(); break; }
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > spin_ms) break;
    }
    HIPCK(hipStreamSynchronize(st));
    return 0;
}

// ---- RCCL, loaded on demand (single-GPU use needs no communicator library) -------
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
static Rccl g_rccl;
static int load_rccl() {
    if (g_rccl.lib) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* lib = nullptr;
    for (const char* n : names) {
        lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (lib) break;
    }
    if (!lib) return fail(std::string("cannot load RCCL: ") + dlerror());
#define SYM(f)                                                          \
    g_rccl.f = reinterpret_cast<decltype(g_rccl.f)>(dlsym(lib, "nccl" #f)); \
    if (!g_rccl.f) return fail("RCCL symbol nccl" #f " missing");
    SYM(GetUniqueId) SYM(CommInitRank) SYM(AllGather) SYM(AllReduce) SYM(CommDestroy) SYM(GetErrorString)
#undef SYM
    g_rccl.lib = lib;
    return 0;
}
#define NCCLCK(expr)                                                                              \
    do {                                                                                          \
        ncclResult_t _r = (expr);                                                                 \
        if (_r != ncclSuccess) return fail(std::string(#expr) + " failed: " + g_rccl.GetErrorString(_r)); \
    } while (0)

// ---- kernel dispatch ---------------------------------------------------------------
typedef void (*PhaseLaunch)(const PhaseArgs&, hipStream_t);
typedef void (*FusedLaunch)(const PhaseArgs&, int flavour, hipStream_t);      // an update launch: the flavour prepare_generation chose for it (kernels.h: Flavour)
typedef void (*EvalLaunch)(const double*, uint32_t, uint32_t, uint32_t, const double*, double*, hipStream_t);

// What the functions of the generation loop (run_generations -> group_generation -> prepare_generation / finish_generation -> the launch_*
// templates; build_window, launch_cr_final, launch_push_sync, push_barrier, push_gen_sums, launch_arena_probe, bpm_push_selftest) tell each other
// about WHERE and HOW the current launches go: one instance per thread, grouped by lifetime.  A DispatchScope (below) is open while any of it is
// set and puts everything but the carried flag and the counters back to idle on every way out; an OnHipStream takes a piece of work to the HIP
// stream for a moment.  Outside a scope the state is idle: `dq` is null and every launch goes to the sampler's HIP stream.
struct bpm_sampler;
struct Dispatch {
    // ---- per bpm_step call (run_generations)
    // the host-callback sampler whose generation loop the update kernel compiled around its HIP-source likelihood is driving (else nullptr):
    // prepare_generation asks who drives a host-callback sampler
    bpm_sampler* user_cur = nullptr;
    bool user_launch_failed = false;       // launch_user_fused found no module to launch from: run_generations reports it

    // ---- per generation
    // Direct mode (aql_queue.h): while run_generations has the sampler in direct mode, dq names its queue and every kernel of the
    // generation loop -- update kernels here, table builds in build_window -- is dispatched by a packet this library writes itself.
    bpm::DirectQueue* dq = nullptr;
    // A local group whose ranks each have a queue of their own (BPM_TEST_PATHS=groupqueues) runs in direct mode rank by rank: dq is
    // re-bound to the rank a piece of work belongs to (bind_rank_queue); the ranks' kernels then wait for each other ACROSS queues the way
    // the ranks of a multi-GPU world do.
    bool group_direct = false;
    bool dq_error = false;                 // a dispatch could not be made: run_generations reports it
    // Fences of an update-kernel packet.  A HIP stream puts agent-scope acquire + release around every kernel; the release (write-back of
    // every XCD's L2 at the end of the kernel) is 0.6 us of a 6 us launch period at cfg2.  On the library's own queue the update kernel instead
    // sends what later kernels read -- accepted rows, ln-like, accept counters, during CR adaptation the Welford rows and the CR slots --
    // through write-through stores (PhaseArgs::wt, kernels.h: store_row_wt16) and its packet carries the acquire only; history rows
    // (non-temporal stores, read by nobody before the drain) are written back by the fenced empty kernel DirectQueue::drain puts behind
    // such packets.  Round 2 did this in the steady state up to 4 MiB per half generation only (two 8-byte atomic stores per lane cost
    // more than the release beyond that, and in burn-in); with one 16-byte store per lane it wins everywhere (profiles/r03_write_through_16B.txt).
    // bpm_set_launch_path(h, 1, 3): acquire + release on every packet with plain stores.  The packet after a table build or after entering
    // direct mode always acquires.
    int update_fence = bpm::DirectQueue::FENCED;
    bool wt_stores = false;                // this generation's update kernels store through (PhaseArgs::wt)
    bool call_last_gen = false;            // the generation being run is the last one of the bpm_step call (its fold is dispatched) ...
    bool dq_call_last_gen = false;         // ... and runs in direct mode: its last update dispatch carries the release (release_this)

    // ---- one-shot: riders on the NEXT update launch, consumed by it (update_packet / take_stop_event)
    // bpm_step_timed: the launch carries this event as its stop event (hipExtLaunchKernelGGL binds it to the dispatch itself: its time stamp
    // is the kernel's end, and no marker packet enters the queue) ...
    hipEvent_t stop_event = nullptr;
    int sig = -1;                          // ... or, on the library's own queue, this timing signal
    bool release_this = false;             // the packet carries the release: the drain that usually follows the call then needs no fence
                                           // kernel (2.5 us of a short window)
    // the packet acquires whatever update_fence says: set by what went onto the queue beside the update kernels (a table build, the running-moment
    // sums, a push barrier, a section on the HIP stream, entering direct mode), cleared by the CR reduction, whose packets all acquire themselves.
    // The one rider that is CARRIED from a generation to the next -- a side kernel at the end of a generation marks the first update packet of the
    // following one -- so no scope resets it.
    bool need_acquire = false;

    // ---- per-thread counters, never reset: update-kernel dispatches by path (bpm_get_launch_stats) and altogether (bpm_step_timed)
    int64_t n_direct = 0, n_stream = 0;
    int64_t timed_launches = 0;

    void mark_acquire(bool v) { need_acquire = v; }
    // everything a DispatchScope owns, back to idle
    void idle() {
        user_cur = nullptr; user_launch_failed = false;
        dq = nullptr; group_direct = false; dq_error = false; update_fence = bpm::DirectQueue::FENCED;
        wt_stores = false; call_last_gen = false; dq_call_last_gen = false;
        stop_event = nullptr; sig = -1; release_this = false;
    }
};
static thread_local Dispatch g_disp;
// Open around one generation (or one chunk of generations under the sparse exchange) of run_generations and around the arena part of
// bpm_push_selftest: whatever way the function is left, the next entry point of this thread finds the state idle.
struct DispatchScope {
    Dispatch& d;
    explicit DispatchScope(bpm_sampler* user_cur = nullptr) : d(g_disp) { d.user_cur = user_cur; }
    ~DispatchScope() { d.idle(); }
    DispatchScope(const DispatchScope&) = delete;
    DispatchScope& operator=(const DispatchScope&) = delete;
};
// "Run this on the HIP stream for a moment" inside a direct-mode generation (the outlier check): the queue binding is set aside and comes back.
struct OnHipStream {
    Dispatch& d;
    bpm::DirectQueue* const dq;
    const bool group_direct;
    OnHipStream() : d(g_disp), dq(d.dq), group_direct(d.group_direct) { d.dq = nullptr; d.group_direct = false; }
    ~OnHipStream() { d.dq = dq; d.group_direct = group_direct; }
    OnHipStream(const OnHipStream&) = delete;
    OnHipStream& operator=(const OnHipStream&) = delete;
};
// The one consumer of the rider of an update launch on the HIP stream (update_packet, below, is that of the riders of a packet)
static inline hipEvent_t take_stop_event(Dispatch& d) {
    hipEvent_t e = d.stop_event;
    d.stop_event = nullptr;
    return e;
}
// The kernel-argument block of a kernel with parameters P... as the device reads it: every parameter at the next offset aligned to its own
// alignment; the block ends at the last parameter's end rounded up to the largest alignment among them.
template <class... P>
struct KernargLayout {
    static constexpr size_t n = sizeof...(P);
    size_t off[n] = {}, size[n] = {sizeof(P)...}, bytes = 0;
    constexpr KernargLayout() {
        constexpr size_t al[n] = {alignof(P)...};
        size_t end = 0, al_max = 1;
        for (size_t i = 0; i < n; ++i) {
            off[i] = (end + al[i] - 1) / al[i] * al[i];
            end = off[i] + size[i];
            al_max = std::max(al_max, al[i]);
        }
        bytes = (end + al_max - 1) / al_max * al_max;
    }
};
// A kernel BESIDE the update kernels (table builds, the CR reduction, the running-moment sums, the push barrier, the arena probe): a packet on the
// queue of the generation being run where one is bound (g_disp.dq), else a launch on `stream`.  The arguments are converted to the kernel's own
// parameter types on either path, and the packet's argument block is laid out from those types: no hand-made mirror of a signature to keep in step.
// (What must stay on the HIP stream WHILE a queue is bound -- see build_window -- launches there itself and never comes here.)
// then: what the launch means for the next update packet -- it must acquire, need not (the CR fold: see need_acquire), or no change.
enum class Then { KEEP, ACQUIRE, NO_ACQUIRE };
template <class... P>
static int launch_side(hipStream_t stream, void (*kernel)(P...), const char* name, dim3 grid, uint32_t block, int fence, Then then, std::common_type_t<P>... args) {
    Dispatch& d = g_disp;
    if (!d.dq) {
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, stream, args...);
        HIPCK(hipGetLastError());
        return 0;
    }
    constexpr KernargLayout<P...> lay;
    alignas(16) unsigned char ka[lay.bytes] = {};
    size_t i = 0;
    ((void)std::memcpy(ka + lay.off[i++], &args, sizeof(P)), ...);
    const bpm::DqKernel* k = d.dq->kernel(reinterpret_cast<const void*>(kernel));
    if (!k || d.dq->launch(*k, grid.x, grid.y, block, ka, lay.bytes, fence) != 0) return fail(std::string("direct AQL queue: ") + name + ": " + d.dq->why());
    if (then != Then::KEEP) d.mark_acquire(then == Then::ACQUIRE);
    return 0;
}
// A kernel of a module compiled at run time (user_likelihood.h, derived.h), on `stream`: K is its parameter list as a function type, declared once
// beside the header that holds the kernel; the arguments are converted to exactly those types and the array of pointers is laid out from them.
template <class K>
struct ModuleLaunch;
template <class... P>
struct ModuleLaunch<void(P...)> {
    static hipError_t on(hipStream_t stream, hipFunction_t fn, unsigned grid, unsigned block, unsigned lds_bytes, std::common_type_t<P>... args) {
        void* ptrs[] = {static_cast<void*>(&args)...};
        return hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, lds_bytes, stream, ptrs, nullptr);
    }
};
static inline uint32_t grid_for(uint32_t n_items, int lpc) {
    const uint32_t cpw = (uint32_t)(block_for(lpc) / lpc);
    return (n_items + cpw - 1) / cpw;
}
// The kernel-argument block of phase_fused_kernel exactly as the device reads it (natural alignment = the kernarg layout): the
// launch goes through hipExtModuleLaunchKernel with this buffer -- no per-launch symbol lookup, no per-argument marshalling.
struct FusedKernarg {
    const uint32_t* pl_plan;
    uint32_t pl_upd_off, pl_n_items, pl_mode, _pad;
    PhaseArgs a;
};
static_assert(offsetof(FusedKernarg, a) == 24 && sizeof(FusedKernarg) == 24 + sizeof(PhaseArgs), "kernarg layout of phase_fused_kernel");
// The hot block of the argument block (kernels.h: PhaseArgs), pinned: kernarg slots are 64-byte aligned (aql_queue.h: SLOT_BYTES), so behind the 24 bytes
// of leading arguments the block's lines end at 40, 104, 168 and 232 -- the same offsets in every build variant.
#define BPM_HOT_AT(field, off) static_assert(offsetof(PhaseArgs, field) == (off), "hot block of PhaseArgs: " #field)
BPM_HOT_AT(L_G, 0); BPM_HOT_AT(L_ld, 8); BPM_HOT_AT(L_dim, 12); BPM_HOT_AT(ll, 16); BPM_HOT_AT(acc_count, 24); BPM_HOT_AT(tparams, 32); BPM_HOT_AT(counters, 40);
BPM_HOT_AT(hist_row, 48); BPM_HOT_AT(llhist_row, 56); BPM_HOT_AT(seed, 64); BPM_HOT_AT(t, 72); BPM_HOT_AT(k, 80); BPM_HOT_AT(upd_off, 84); BPM_HOT_AT(epsilon, 88);
BPM_HOT_AT(wt, 96); BPM_HOT_AT(hist_by_pos, 100);                                                                                  // every planned flavour: lines 0, 1
BPM_HOT_AT(cr_state, 104); BPM_HOT_AT(gamma_tab, 112); BPM_HOT_AT(u_epsilon, 120); BPM_HOT_AT(w_mean, 128); BPM_HOT_AT(w_m2, 136); BPM_HOT_AT(cr_gate, 144);
BPM_HOT_AT(hist_len, 148); BPM_HOT_AT(thr, 152);                                                                                   // DREAM, its burn-in: line 2
BPM_HOT_AT(L_blk, 184); BPM_HOT_AT(L_n_local, 192); BPM_HOT_AT(L_world, 196); BPM_HOT_AT(L_magic, 200); BPM_HOT_AT(lo, 204);
BPM_HOT_AT(gamma_demc, 208); BPM_HOT_AT(p_snooker, 216); BPM_HOT_AT(M, 224); BPM_HOT_AT(pool_off, 228);                            // a rank of a world, DE-MC: line 3
#undef BPM_HOT_AT
static_assert((offsetof(FusedKernarg, a) + offsetof(PhaseArgs, thr) + 4 * sizeof(uint32_t)) % 64 == 0 && (offsetof(FusedKernarg, a) + offsetof(PhaseArgs, pool_off) + sizeof(uint32_t)) % 64 == 0 &&
              bpm::DirectQueue::SLOT_BYTES % 64 == 0, "the hot block's lines 2 and 3 end on lines of the kernarg segment");
// One update-kernel dispatch from a ready argument block (a FusedKernarg, or the bare PhaseArgs a run-time module's kernels take) and the counters
// it moves: as a packet on the library's own queue (k: null = the kernel was not found), the one consumer of a packet's riders -- its fences and
// its timing signal, what it used cleared ...
static inline void update_packet(Dispatch& d, const bpm::DqKernel* k, unsigned grid, unsigned block, const void* ka, size_t nbytes) {
    int fence = d.update_fence;
    const int sig = d.sig;
    d.sig = -1;
    if (d.need_acquire) { fence |= bpm::DirectQueue::ACQUIRE; d.need_acquire = false; }
    if (d.release_this) { fence |= bpm::DirectQueue::RELEASE; d.release_this = false; }
    if (!k || d.dq->launch(*k, grid, 1, block, ka, nbytes, fence, sig) != 0) d.dq_error = true;
    ++d.timed_launches; ++d.n_direct;
}
// ... or from a module function on the HIP stream
static inline void update_on_stream(Dispatch& d, hipFunction_t fn, unsigned grid, unsigned block, void* ka, size_t nbytes, hipStream_t s) {
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &nbytes, HIP_LAUNCH_PARAM_END};
    (void)hipExtModuleLaunchKernel(fn, grid * block, 1, 1, block, 1, 1, 0, s, nullptr, extra, nullptr, take_stop_event(d), 0);
    ++d.timed_launches; ++d.n_stream;
}
template <class K>
static inline void launch_packed(K kernel, hipFunction_t& fn, const PhaseArgs& a, unsigned grid, unsigned block, hipStream_t s) {
    Dispatch& d = g_disp;
    FusedKernarg ka{a.rec_tab, a.rec_off, a.n_items, a.mode, 0u, a};
    if (d.dq) return update_packet(d, d.dq->kernel(reinterpret_cast<const void*>(kernel)), grid, block, &ka, sizeof(ka));
    if (!fn) { if (hipGetFuncBySymbol(&fn, reinterpret_cast<const void*>(kernel)) != hipSuccess) { (void)hipGetLastError(); fn = nullptr; } }
    if (fn) return update_on_stream(d, fn, grid, block, &ka, sizeof(ka), s);
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, nullptr, take_stop_event(d), 0, a.rec_tab, a.rec_off, a.n_items, a.mode, a);
    ++d.timed_launches; ++d.n_stream;
}
template <int ALGO, int T, int NP, int LPC, int DPL, int HOT>
static void launch_hot(const PhaseArgs& a, hipStream_t s) {
    static hipFunction_t fn = nullptr;
    constexpr unsigned blk = (unsigned)block_for_hot(LPC, HOT, DPL), cpw = blk / (unsigned)LPC;      // (burn-in flavours of one wavefront per chain: 16 chains per workgroup)
    launch_packed(phase_fused_kernel<ALGO, T, LPC, DPL, NP, HOT>, fn, a, (a.n_items + cpw - 1u) / cpw, blk, s);
}
// The instantiation of the flavour chosen for the launch (prepare_generation; kernels.h: choose_flavour): same argument block, same two launch paths
// for all of them.  A shape has the flavours choose_flavour can return for it: those with plan records only where the shape can read them, the
// burn-in ones only for DREAM.
template <int ALGO, int T, int NP, int LPC, int DPL>
static void launch_fused(const PhaseArgs& a, int flavour, hipStream_t s) {
    constexpr bool CAN_PLAN = (LPC == WAVE && DPL == 2), DREAM_ = ALGO == ALGO_DREAM;
    switch (flavour) {
        case FLAVOUR_STEADY_PLAN: if constexpr (CAN_PLAN) return launch_hot<ALGO, T, NP, LPC, DPL, FLAVOUR_STEADY_PLAN>(a, s); break;
        case FLAVOUR_STEADY: return launch_hot<ALGO, T, NP, LPC, DPL, FLAVOUR_STEADY>(a, s);
        case FLAVOUR_ADAPT_PLAN: if constexpr (CAN_PLAN && DREAM_) return launch_hot<ALGO, T, NP, LPC, DPL, FLAVOUR_ADAPT_PLAN>(a, s); break;
        case FLAVOUR_ADAPT: if constexpr (DREAM_) return launch_hot<ALGO, T, NP, LPC, DPL, FLAVOUR_ADAPT>(a, s); break;
        case FLAVOUR_SHARD_PLAN: if constexpr (CAN_PLAN) return launch_hot<ALGO, T, NP, LPC, DPL, FLAVOUR_SHARD_PLAN>(a, s); break;
        default: break;
    }
    launch_hot<ALGO, T, NP, LPC, DPL, FLAVOUR_GENERAL>(a, s);
}
template <int ALGO, int LPC, int DPL>
static void launch_propose(const PhaseArgs& a, hipStream_t s) {
    // the usual pair counts as compile-time constants (DREAM's default 3, DE-MC's 1): the partner ids stay in registers (kernels.h: phase_propose_kernel)
    constexpr int NPC = ALGO == ALGO_DREAM ? 3 : 1;
    if (a.mode != 2u && a.P == (uint32_t)NPC && !(ALGO != ALGO_DREAM && a.p_snooker > 0.0))
        hipLaunchKernelGGL((phase_propose_kernel<ALGO, LPC, DPL, NPC>), dim3(grid_for(a.n_items, LPC)), dim3(block_for(LPC)), 0, s, a);
    else
        hipLaunchKernelGGL((phase_propose_kernel<ALGO, LPC, DPL>), dim3(grid_for(a.n_items, LPC)), dim3(block_for(LPC)), 0, s, a);
}
template <int ALGO, int LPC, int DPL>
static void launch_commit(const PhaseArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((phase_commit_kernel<ALGO, LPC, DPL>), dim3(grid_for(a.n_items, LPC)), dim3(block_for(LPC)), 0, s, a);
}
template <int T, int LPC, int DPL>
static void launch_eval(const double* X, uint32_t n, uint32_t ld, uint32_t dim, const double* tp, double* out,
                        hipStream_t s) {
    hipLaunchKernelGGL((eval_ll_kernel<T, LPC, DPL>), dim3(grid_for(n, LPC)), dim3(block_for(LPC)), 0, s, X, n, ld, dim, tp, out);
}

struct Shape {
    int lpc, dpl, idx;
};
// lanes per chain / coordinates per lane for a row of ld doubles (ld even)
static bool pick_shape(uint32_t ld, Shape& sh) {
    const uint32_t np = ld / 2;
    if (np <= 1) sh = {1, 2, 0};
    else if (np <= 4) sh = {4, 2, 1};
    else if (np <= 16) sh = {16, 2, 2};
    else if (np <= 64) sh = {64, 2, 3};   // (two / four chains per wavefront, 32x4 and 16x8, measured no faster: DESIGN.md)
    else if (np <= 128) sh = {64, 4, 4};
    else if (np <= 256) sh = {64, 8, 5};
    // d > 512: one wavefront per chain LOOPING over the row (kernels_wide.h) -- no dimension limit, no scratch.  (Round 3 had 16 and 32 coordinates
    // per lane for d <= 1024 / 2048: the looped kernel is faster than the first -- 0.71 / 0.74 / 0.76 of the HBM roof at d = 640 / 1000 / 1024 against
    // 0.56 / 0.71 / 0.74 -- and replaces the second, which spilled: profiles/r04_wide_rows.txt.)
    else sh = {64, 0, 6};
    return true;
}
constexpr int SHAPE_WIDE = 6;
// [shape]: the register-resident kernels by (lanes per chain, coordinates per lane), then the looped wide-row kernel
#define SHAPE_TABLE(FN, WIDE, ...)                                                               \
    {FN<__VA_ARGS__ 1, 2>, FN<__VA_ARGS__ 4, 2>, FN<__VA_ARGS__ 16, 2>, FN<__VA_ARGS__ 64, 2>, \
     FN<__VA_ARGS__ 64, 4>, FN<__VA_ARGS__ 64, 8>, WIDE}
#define COMMA ,
// ---- the looped wide-row kernels (kernels_wide.h): same argument block and launch paths as phase_fused_kernel
template <int ALGO, int T, int NP>
static void launch_wide(const PhaseArgs& a, int, hipStream_t s) {      // (one flavour: the general one)
    const unsigned grid = (unsigned)((a.n_items + (BPM_BLOCK_WAVE / WAVE) - 1) / (BPM_BLOCK_WAVE / WAVE));
    static hipFunction_t fn = nullptr;
    launch_packed(phase_wide_kernel<ALGO, T, NP, STAGE_FUSED>, fn, a, grid, (unsigned)BPM_BLOCK_WAVE, s);
}
template <int ALGO>
static void launch_wide_propose(const PhaseArgs& a, hipStream_t s) {
    const unsigned grid = (unsigned)((a.n_items + (BPM_BLOCK_WAVE / WAVE) - 1) / (BPM_BLOCK_WAVE / WAVE));
    hipLaunchKernelGGL((phase_wide_kernel<ALGO, TARGET_HOST, 0, STAGE_PROPOSE>), dim3(grid), dim3(BPM_BLOCK_WAVE), 0, s, a.rec_tab, a.rec_off, a.n_items, a.mode, a);
}
template <int ALGO>
static void launch_wide_commit(const PhaseArgs& a, hipStream_t s) {
    const unsigned grid = (unsigned)((a.n_items + (BPM_BLOCK_WAVE / WAVE) - 1) / (BPM_BLOCK_WAVE / WAVE));
    hipLaunchKernelGGL((phase_wide_commit_kernel<ALGO>), dim3(grid), dim3(BPM_BLOCK_WAVE), 0, s, a);
}
template <int T>
static void launch_eval_wide(const double* X, uint32_t n, uint32_t ld, uint32_t dim, const double* tp, double* out, hipStream_t s) {
    hipLaunchKernelGGL((eval_ll_wide_kernel<T>), dim3((n + (BPM_BLOCK_WAVE / WAVE) - 1) / (BPM_BLOCK_WAVE / WAVE)), dim3(BPM_BLOCK_WAVE), 0, s, X, n, ld, dim, tp, out);
}
// update-kernel variants: [DE-MC (1 pair) | DREAM del_pairs = 3 (compile-time) | DREAM any del_pairs][shape]
static FusedLaunch g_fused_gauss[3][7] = {SHAPE_TABLE(launch_fused, launch_wide<ALGO_DEMC COMMA TARGET_GAUSS COMMA 1>, ALGO_DEMC COMMA TARGET_GAUSS COMMA 1 COMMA),
                                          SHAPE_TABLE(launch_fused, launch_wide<ALGO_DREAM COMMA TARGET_GAUSS COMMA 3>, ALGO_DREAM COMMA TARGET_GAUSS COMMA 3 COMMA),
                                          SHAPE_TABLE(launch_fused, launch_wide<ALGO_DREAM COMMA TARGET_GAUSS COMMA 0>, ALGO_DREAM COMMA TARGET_GAUSS COMMA 0 COMMA)};
static FusedLaunch g_fused_mixture[3][7] = {SHAPE_TABLE(launch_fused, launch_wide<ALGO_DEMC COMMA TARGET_MIXTURE COMMA 1>, ALGO_DEMC COMMA TARGET_MIXTURE COMMA 1 COMMA),
                                            SHAPE_TABLE(launch_fused, launch_wide<ALGO_DREAM COMMA TARGET_MIXTURE COMMA 3>, ALGO_DREAM COMMA TARGET_MIXTURE COMMA 3 COMMA),
                                            SHAPE_TABLE(launch_fused, launch_wide<ALGO_DREAM COMMA TARGET_MIXTURE COMMA 0>, ALGO_DREAM COMMA TARGET_MIXTURE COMMA 0 COMMA)};
static FusedLaunch g_fused_banana[3] = {launch_fused<ALGO_DEMC, TARGET_BANANA, 1, 1, 2>, launch_fused<ALGO_DREAM, TARGET_BANANA, 3, 1, 2>,
                                        launch_fused<ALGO_DREAM, TARGET_BANANA, 0, 1, 2>};
static PhaseLaunch g_propose[2][7] = {SHAPE_TABLE(launch_propose, launch_wide_propose<ALGO_DEMC>, ALGO_DEMC COMMA),
                                      SHAPE_TABLE(launch_propose, launch_wide_propose<ALGO_DREAM>, ALGO_DREAM COMMA)};
template <int ALGO, int NP, int LPC, int DPL>
static void launch_replay(const PhaseArgs& a, hipStream_t s) {
    // (a workgroup per 64 positions that compacts the remote accepted chains in LDS and rebuilds only those -- 8192 wavefronts
    // launched instead of 32768 -- measured no faster: 11.5 vs 11.3 us at 8 ranks, 6.9 vs 5.2 at 2; profiles/r02_replay_variants.txt)
    hipLaunchKernelGGL((phase_replay_kernel<ALGO, LPC, DPL, NP>), dim3(grid_for(a.n_upd, LPC)), dim3(block_for(LPC)), 0, s, a);
}
template <int ALGO, int NP, int DPL>
static void launch_replay_sorted(const PhaseArgs& a, hipStream_t s) {
    uint32_t max_cnt = 0;                                     // the largest count among the OTHER ranks' updates of this half generation
    for (uint32_t r = 0; r < a.n_seg; ++r)
        if (r != a.seg_me) max_cnt = std::max(max_cnt, a.seg_off[r + 1] - a.seg_off[r]);
    if (max_cnt == 0) return;
    hipLaunchKernelGGL((phase_replay_sorted_kernel<ALGO, DPL, NP>), dim3((max_cnt + REPLAY_WG / WAVE - 1) / (REPLAY_WG / WAVE), a.n_seg), dim3(REPLAY_WG),
                       0, s, a);
}
// [DE-MC | DREAM del_pairs = 3 | DREAM any del_pairs][dims per lane 2 / 4 / 8]: owner-sorted records exist for one wavefront per chain only
#define RS_ROW(A, P) {launch_replay_sorted<A, P, 2>, launch_replay_sorted<A, P, 4>, launch_replay_sorted<A, P, 8>}
static PhaseLaunch g_replay_sorted[3][3] = {RS_ROW(ALGO_DEMC, 1), RS_ROW(ALGO_DREAM, 3), RS_ROW(ALGO_DREAM, 0)};
// [DE-MC | DREAM del_pairs = 3 | DREAM any del_pairs][shape]: the same pair-count variants as the update kernels (no target: no ln-like)
// (wide rows have no replay kernel: a world of wide-row samplers exchanges by push or by the dense all-gather -- bpm_set_exchange refuses the rest)
static PhaseLaunch g_replay[3][7] = {SHAPE_TABLE(launch_replay, nullptr, ALGO_DEMC COMMA 1 COMMA), SHAPE_TABLE(launch_replay, nullptr, ALGO_DREAM COMMA 3 COMMA),
                                     SHAPE_TABLE(launch_replay, nullptr, ALGO_DREAM COMMA 0 COMMA)};
static PhaseLaunch g_commit[2][7] = {SHAPE_TABLE(launch_commit, launch_wide_commit<ALGO_DEMC>, ALGO_DEMC COMMA),
                                     SHAPE_TABLE(launch_commit, launch_wide_commit<ALGO_DREAM>, ALGO_DREAM COMMA)};
static EvalLaunch g_eval_gauss[7] = SHAPE_TABLE(launch_eval, launch_eval_wide<TARGET_GAUSS>, TARGET_GAUSS COMMA);
static EvalLaunch g_eval_mixture[7] = SHAPE_TABLE(launch_eval, launch_eval_wide<TARGET_MIXTURE>, TARGET_MIXTURE COMMA);

// "The history is still what the first call of a pair saw" (bpm_diag_split_moments -> bpm_diag_autocov, bpm_quantile_begin ->
// bpm_quantile_histogram, bpm_hist_range -> bpm_hist_marginals / bpm_hist_pairs, bpm_trace_bins -> bpm_trace_chains): the first call take()s,
// the ones that follow check().
struct bpm_sampler;
struct HistorySnapshot {
    bool valid = false;
    uint64_t epoch = 0;
    int64_t tabs = 0, rows = 0;
    void take(const bpm_sampler* s);
    int check(const bpm_sampler* s, const char* who, const char* first_call) const;
};

#include "device_memory.h"      // MemKind, DevTemp, MemRegistry: the only code that allocates or frees device and pinned host memory

// ---- what a program compiled at run time leaves on the device: owned from the moment it exists ------------------------------------------
// A loaded code object: unloaded when its owner goes, unless leak()ed (bpm_destroy under a queue that may still run kernels).  The one place
// that loads, looks up and unloads.
struct Module {
    hipModule_t mod = nullptr;
    Module() = default;
    Module(Module&& o) noexcept : mod(o.mod) { o.mod = nullptr; }
    Module& operator=(Module&& o) noexcept {
        if (this != &o) { unload(); mod = o.mod; o.mod = nullptr; }
        return *this;
    }
    ~Module() { unload(); }
    hipError_t load(const std::vector<char>& code) { unload(); return hipModuleLoadData(&mod, code.data()); }
    hipFunction_t function(const std::string& name) const {      // null: not there (the HIP error is cleared)
        hipFunction_t fn = nullptr;
        if (hipModuleGetFunction(&fn, mod, name.c_str()) == hipSuccess && fn) return fn;
        (void)hipGetLastError();
        return nullptr;
    }
    void unload() { if (mod) (void)hipModuleUnload(mod); mod = nullptr; }
    void leak() { mod = nullptr; }
};
// A caller's parameter block on the device: max(n, 1) doubles, zero-filled, then the caller's n -- enqueued on `stream`; the caller's array is
// its own again once that stream has been waited for.
struct DevParams : DevTemp<double> {
    int upload(const double* src, int32_t n, hipStream_t stream) {
        CK(alloc((size_t)std::max(n, 1)));
        HIPCK(hipMemsetAsync(p, 0, (size_t)std::max(n, 1) * sizeof(double), stream));
        if (n > 0) HIPCK(hipMemcpyAsync(p, src, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream));
        return 0;
    }
};
// ---- the one way a caller's source becomes an installed function (the likelihood, the derived function, the pointwise density, PSIS-LOO's stages) ----
// the arch a run-time program is compiled for: the device's own
static int device_arch(int device, std::string& arch) {
    hipDeviceProp_t prop;
    HIPCK(hipGetDeviceProperties(&prop, device));
    arch = prop.gcnArchName;
    return 0;
}
// What a compile_* wrapper returned (`why`: "" or the reason, `code`) loaded into `mod` and its kernels looked up by name
struct KernelSlot { const char* name; hipFunction_t* fn; };
static int load_kernels(const std::string& who, const std::string& why, const std::vector<char>& code, Module& mod, std::initializer_list<KernelSlot> kernels) {
    if (!why.empty()) return fail(who + ": " + why);
    HIPCK(mod.load(code));
    for (const KernelSlot& k : kernels)
        if (!(*k.fn = mod.function(k.name))) return fail(who + ": the compiled module has no " + k.name + " kernel");
    return 0;
}
// ... compiled for `device` first: compile(arch, code) -> "" or the reason
template <class Compile>
static int compile_and_load(const std::string& who, int device, Compile compile, Module& mod, std::initializer_list<KernelSlot> kernels) {
    std::string arch;
    std::vector<char> code;
    CK(device_arch(device, arch));
    return load_kernels(who, compile(arch, code), code, mod, kernels);
}
// Compile only, no device (bpm_check_*): the reason goes into `log` too.  args_ok(): the check of the entry point's other arguments (0 or its
// fail()), made after the null source's.
template <class ArgsOk, class Compile>
static int check_source(const std::string& who, const char* hip_source, const char* arch, char* log, int64_t log_cap, ArgsOk args_ok, Compile compile) {
    if (!hip_source) return fail(who + ": null source");
    CK(args_ok());
    std::vector<char> code;
    const std::string why = compile((arch && *arch) ? arch : "gfx950", code);
    bpm::copy_text(why, log, log_cap);
    return why.empty() ? 0 : fail(who + ": " + why);
}
// THE INSTALL CONTRACT.  The new function is built beside the installed one (build(next): compile_and_load, whatever it owns on the device), its
// parameters are uploaded and the stream is waited for -- a previous function's launches are done, the caller's arrays are its own again.  Only
// then, when nothing can fail any more, does it take the installed one's place (retire(installed) first): an error on the way leaves the installed
// function whole.  same: the installed one was built from this source and shape already -- the parameters only.
template <class F, class Build, class Retire = void (*)(F&)>
static int install_function(hipStream_t stream, F& installed, bool same, const double* params, int32_t n_params, Build build, Retire retire = [](F&) {}) {
    F next;
    if (!same) CK(build(next));
    CK(next.params.upload(params, n_params, stream));
    HIPCK(hipStreamSynchronize(stream));
    if (same) { installed.params = std::move(next.params); return 0; }
    retire(installed);
    installed = std::move(next);
    return 0;
}
// The caller's ln_like_fn as a kernel compiled from HIP source (user_likelihood.h; bpm_set_device_likelihood): bpm_step then drives a host-callback sampler ...
struct UserLikelihood {
    Module mod;
    hipFunction_t fn = nullptr;              // bpm_user_eval
    DevParams params;
    // ... and the update kernel itself compiled around it (user_likelihood.h: compile_user_fused): one launch per half generation; fn == nullptr: the three-kernel form
    struct Fused {
        Module mod;
        hipFunction_t fn = nullptr;          // the general instantiation
        hipFunction_t hot = nullptr;         // the steady-state one (HOT 1 with update records, 2 without: compiled for what the sampler builds)
        hipFunction_t eval = nullptr;        // eval_ll_kernel with the same target: the current states' ln-likes by the update kernel's own arithmetic
        hipFunction_t adapt = nullptr;       // DREAM's burn-in instantiation (HOT 3 / 4): level 1 of the CR reduction and the consumer-side fold inside the launch
        unsigned block = 0, block_adapt = 0;
        std::string names[3];                // their lowered names ([2]: the burn-in instantiation): what the library's own queue dispatches them by (DirectQueue::kernel_by_name)
        bool dq = false;                     // ... and all were found among the loaded code objects
        // the one way out: the queue forgets the names, then the module is unloaded
        void drop(bpm::DirectQueue* q) {
            if (mod.mod && q) for (const std::string& nm : names) q->forget_named(nm);
            *this = Fused();
        }
    } fused;
    std::string why;                         // why the fused form is not in use (bpm_get_device_likelihood_info)
    // the PER-DATUM form (user_eval_data.h; bpm_set_device_likelihood_data): fn is bpm_user_eval_data, `fold` bpm_user_fold_data; the caller's data
    // (n_data, w) and the chunk sums [row][chunk][K] of a batch of `batch_rows` rows are the likelihood's own.  n_data == 0: another form.
    hipFunction_t fold = nullptr;
    DevTemp<double> data, part;
    int32_t n_data = 0, n_chunks = 0;
    uint32_t batch_rows = 0;
    void leak() { mod.leak(); params.leak(); fused.mod.leak(); data.leak(); part.leak(); }
};
// A caller's function of one sample, compiled around the window reduction of derived.h (bpm_set_device_function): kept until replaced or bpm_destroy
struct DerivedFunction {
    Module mod;
    hipFunction_t fn = nullptr;              // bpm_derive_rows of THIS module: launched by handle, never looked up by name
    hipFunction_t fill = nullptr;            // bpm_derive_fill of the same module (bpm_derive_history)
    std::string src;                         // the source bytes and n_out the module was built from: the same again only re-upload the parameters
    int32_t n_out = 0;
    DevParams params;
    void leak() { mod.leak(); params.leak(); }
};

// A caller's log density of one datum, compiled around the streaming reduction of pointwise_rows.h (bpm_set_pointwise), with the device copy of the
// caller's data (n_data, w): kept until replaced or bpm_destroy
struct PointwiseFunction {
    Module mod;
    hipFunction_t fn = nullptr;              // bpm_pointwise_rows of THIS module
    std::string src;                         // the source bytes, w and the data the module and the copy were made from: the same again only
    std::vector<double> data_h;              // re-upload the parameters
    int32_t w = 0;
    int64_t n_data = 0;
    DevTemp<double> data;
    DevParams params;
    Module tail_mod;                         // pointwise_tail.h around the same source (bpm_loo compiles it at its first call): stages A and B of PSIS-LOO
    hipFunction_t tail_fn = nullptr, tail_final_fn = nullptr, body_fn = nullptr;
    void leak() { mod.leak(); tail_mod.leak(); data.leak(); params.leak(); }
};

// ---- the sampler ------------------------------------------------------------------------
struct bpm_sampler {
    bpm_config_t cfg{};
    std::vector<double> tparams_h;
    uint32_t N = 0, dim = 0, ld = 0, n_local = 0, lo = 0, world = 1, rank = 0;
    Shape shape{};
    Layout L{};
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    MemRegistry mem;                  // owns every device and pinned host buffer named below
    // bpm_step_timed: ev0 rides on the first update launch of the call, ev1 on the last one
    bool timed_want_first = false;
    int64_t timed_skip = 0;           // update launches to let pass before ev0 is attached (see bpm_step_timed)
    int64_t timed_last_gen = -1;      // t_abs of the call's last generation (-1: not timing)
    int64_t timed_l0 = 0, timed_l1 = 0;   // launch counter values at those two launches
    double* G = nullptr;
    double* ll = nullptr;
    double* hist = nullptr;
    double* llhist = nullptr;
    int64_t hist_cap = 0;      // rows allocated
    // Position-ordered history append (single GPU, fewer than 64 lanes per chain): the update kernels write a generation's history row in
    // that generation's shuffle order -- consecutive work items, consecutive rows: 1.0 us per generation at cfg3, 5.5 us at cfg5 against
    // the scattered append by chain index (profiles/r03_small_d_hops_and_position_order.txt) -- and hist_tag[row] remembers how to read it:
    // -1 chain order, else (generation << 2) | (2: the row's ln-like went by chain all the same) | shuffle.  normalize_history puts rows back into chain
    // order, in place, before anything reads them by chain (bpm_get_history, the moment rebuild, a partial first generation of bpm_reduce_moments);
    // the outlier check reads them where they lie (outlier_row_keys).
    bool hist_by_pos = false;
    std::vector<int64_t> hist_tag;
    PermKey* okeys = nullptr;               // outlier check: per history row the shuffle key of its state row [0, cap) and of its ln-like [cap, 2 cap)
    size_t okeys_cap = 0;                   // (outlier_row_keys)
    std::vector<PermKey> okeys_host;
    bool okeys_x = false, okeys_ll = false; // any state row / any ln-like row of the history still lies in position order
    uint32_t* olist = nullptr;              // outlier check: [0] count, then the local chains that were reset (outlier_rebuild_kernel)
    double* hist_tmp = nullptr;    // one row (n_local * ld) + its ln-likes (n_local): staging of normalize_history
    int64_t hist_rows = 0;     // rows stored (0 when keep_history == 0 and nothing stored)
    int64_t rows_logical = 0;  // len(chain.chain) of the reference: 1 + generations since (re)initialisation
    // Thinned history (bpm_set_history_thin / bpm_thin_history): stored row r is logical row r * hist_stride, a generation is appended iff the logical
    // row it produces is a multiple of the stride.  A property of the handle: (re)initialisation keeps it.  1: a row per generation (chain.py:51-54).
    int64_t hist_stride = 1;
    // running population sums (cfg.running_moments): per history row g the 2 ld doubles [sum_i (x_ij - shift_j) | sum_i (x_ij - shift_j)^2]
    // over this rank's chains, shift = chain 0's state at the last (re)initialisation.  bpm_reduce_moments answers from them when
    // the history is not resident: param_est (demc.py:235-248) of 10^5 generations of config 2 without 660 GB of history.
    double* gen_sums = nullptr;
    int64_t gen_sums_cap = 0;      // rows allocated
    double* gs_shift = nullptr;    // [ld]
    double* gs_part = nullptr;     // per-block partial sums of one row
    uint32_t gs_nb = 0;
    double* w_mean = nullptr;
    double* w_m2 = nullptr;
    int64_t w_rows = 0;        // history rows folded into the Welford moments
    double* tparams = nullptr;
    double* cr_state = nullptr;       // the CURRENT totals block p_cr | delta_m | n_cr_updates: one of the two halves of cr_state_base (cr_state_alt the other)
    double* cr_state_alt = nullptr;
    double* cr_state_base = nullptr;
    // CR reduction (kernels.h): level-1 partial sums [2 MAX_CR][cr_n1] of a generation (chunks of cr_g1 positions), two buffers for the cr_mid_kernel passes
    double* cr_p1 = nullptr;          // two generations' worth: generation t writes half t & 1 (cr_p1_cur) -- the update kernel that folds generation t's sums
    double* cr_p1_cur = nullptr;      // (consumer-side fold, below) writes its own level 1 in the same launch
    // Consumer-side fold (round 5): where the update kernels sum level 1 themselves (one GPU, HOT 3 / 4) a generation's fold is NOT dispatched (cr_final_kernel:
    // one wavefront at the floor of a dependent launch, 4.5 us of cfg2's 20.6 us burn-in generation): it stays pending, and every workgroup of the NEXT
    // generation's first update launch folds the sums itself (PhaseArgs::cr_fold_part: a wavefront per array of partial sums, the same additions in the same order), workgroup 0 stores
    // the new totals into the other totals block, which the second launch and everything later read.  What cannot consume a pending fold -- the last generation
    // of a bpm_step call, the first steady-state generation, a launch of another flavour -- gets cr_final_kernel as before (cr_flush_pending).
    bool cr_pending = false;
    const double* cr_pend_src = nullptr;      // (the generation's level-1 sums, or what the cr_mid_kernel passes left of them: cr_pend_cnt <= CR_FINAL_MAX per array)
    uint32_t cr_pend_cnt = 0;
    double* cr_p2[2] = {nullptr, nullptr};
    uint32_t cr_g1 = 16, cr_n1 = 0;
    bool gen_cr_inkernel = false;     // this generation's update kernels write level 1 themselves (every launch has a burn-in flavour, HOT 3 / 4, of a shape that sums)
    unsigned long long* counters = nullptr;  // device: [2] = NaN ratios
    uint32_t* acc_count = nullptr;           // device: accepted updates per local chain, this run
    int64_t gens_this_run_local = 0;
    double* prop_buf = nullptr;
    // host-callback path: pinned staging of what bpm_propose reads back and bpm_commit sends (work-item order)
    int32_t* h_ids = nullptr;
    double* h_props = nullptr;
    double* h_ll = nullptr;                  // [n_local] ln-likes by work item on their way in (bpm_commit_chunk)
    std::vector<hipEvent_t> chunk_ev;        // one event behind every chunk of the proposals' read-back (bpm_propose_begin)
    int32_t prop_chunks = 0, prop_given = 0; // chunks of the open half generation / chunks whose ln-likes have been handed in
    int prop_mode = 0;                       // how the open half generation was proposed: 1 host staging (chunks), 2 device-resident
    int64_t prop_active = 0;                 // its active work items
    bool prop_whole = false;                 // it was proposed through bpm_propose (caller-owned buffers): bpm_commit finishes it
    std::vector<uint8_t> prop_done;          // [prop_chunks] 1: the piece's ln-likes have been handed in
    UserLikelihood like;                     // the caller's ln_like_fn given as HIP source (bpm_set_device_likelihood)
    DerivedFunction derived;                 // the caller's function of one sample (bpm_set_device_function)
    PointwiseFunction pointwise;             // the caller's log density of one datum and its data (bpm_set_pointwise)
    double* aux_buf = nullptr;
    int32_t* ids_buf = nullptr;
    int32_t* trace_i32 = nullptr;      // per-chain decision trace (bpm_set_trace: test variant only; always null in the product library)
    double* trace_f64 = nullptr;
    uint8_t* trace_mask = nullptr;
    double* scratch = nullptr;   // small device scratch (theta0, var, moments)
    // Per-generation tables that depend only on (seed, generation, N) -- shuffle orders, update records -- are built a WINDOW
    // of win_K generations at a time (window W = generations [W win_K, (W + 1) win_K)) into one of two buffers, one window
    // AHEAD of the update kernels: entering window W enqueues the build of W + 1.  A bpm_step call therefore never starts
    // with a table build (round 1 built the tables of a call at its head: 13 us inside a timed window of 20 generations),
    // and a rank of a world finds the launch sizes of a window on the host without a stall.
    struct TabBuf {
        uint32_t* perm = nullptr;       // [win_K * N] shuffle orders, position -> chain id
        uint32_t* inv = nullptr;        // [win_K * N] chain id -> position
        uint32_t* plan = nullptr;       // [win_K * N * PLAN_WORDS] update records (plan_kernel) or nullptr
        uint32_t* sidx = nullptr;       // world > 1: [win_K * N] slot of every position in the owner-sorted order of its generation (plan_slot_kernel);
                                        // `plan` then holds the records in THAT order (rank segment by rank segment inside each group)
        uint32_t* chunk_count = nullptr; // push exchange: per-chunk counts of this rank's positions (plan_slot_own_kernel)
        uint32_t* plan_count = nullptr; // device [win_K * 2 * world]: updates of every rank in every half generation
        uint32_t* count_h = nullptr;    // the same in pinned host memory, copied behind the build
        bool own_only = false;          // its records cover this rank's chains only (built under the push exchange)
        int64_t W = -1;                 // window held (or being built)
        int shuffle = -1;
        hipEvent_t built = nullptr;     // recorded on the build stream behind the window's last kernel / copy
    };
    TabBuf tb[2];
    int cur = -1;                       // buffer the update stream is using
    int win_K = 0;                      // generations per window (<= PERM_CHUNK)
    bool plan_on = false, sorted_on = false;   // sorted_on: world > 1 with owner-sorted records
    // the current window (aliases into tb[cur])
    uint32_t* perm_tab = nullptr;
    uint32_t* inv_tab = nullptr;
    uint32_t* plan_tab = nullptr;
    const uint32_t* plan_count_h = nullptr;
    int64_t tab_t0 = -1;
    int tab_K = 0;
    int tab_shuffle = -1;
    double* gamma_tab = nullptr;    // [dim + 1]
    double* x_next = nullptr;       // [n_local * ld] banked updates of a synchronous DE-MC generation
    unsigned long long* stamps = nullptr;   // diagnostic build (-DBPM_STAMPS) only
    size_t scratch_doubles = 0;
    ncclComm_t comm = nullptr;
    bool local_group = false;     // test mode: ranks are handles of ONE process, exchanged by device copies
    // push exchange (world > 1): the exchange buffer G, the outlier block om and the control block live in ONE
    // allocation (the arena) that the other ranks map (hipIpcOpenMemHandle); owners push accepted rows into every replica from the
    // update kernel, push_sync_kernel orders the half generations across ranks.  No collective, no replay kernel.
    void* arena = nullptr;
    size_t arena_bytes = 0, off_om = 0, off_ctrl = 0;
    PushCtrl* ctrl = nullptr;
    bool ctrl_fine = false;                 // the control block is a FINE-GRAINED allocation of its own (what a flag polled inside a kernel while
                                            // another agent writes it should live in; inside the coarse-grained arena otherwise)
    void* peer_ctrl_base[MAX_SEG] = {};     // the peers' fine-grained control blocks as this process addresses them
    bool peer_ctrl_opened[MAX_SEG] = {};
    bool push_connected = false, push_enabled = false, push_no_rccl = false;
    bool push_failed = false;      // a cross-rank wait ran into its limit: push cannot be re-enabled (bpm_set_exchange)
    bool push_agent_scope = false;          // update packets fence at agent scope instead of system scope (bpm_set_exchange(h, 3, 1))
    bool probe_sys_ok = false, probe_agent_ok = false, probe_direct = false;   // bpm_push_selftest: the arena probe under system- / agent-scope packet
                                                                               // fences, and whether it ran on the library's own queue
    void* peer_base[MAX_SEG] = {};          // every rank's arena as THIS process addresses it (own entry: arena)
    bool peer_opened[MAX_SEG] = {};         // mapped with hipIpcOpenMemHandle (to be closed)
    unsigned long long* tab_peerG = nullptr;    // device [MAX_PEERS]: G of the other ranks (PhaseArgs::peer_tab)
    unsigned long long* tab_all = nullptr;      // device [3][MAX_SEG]: G | ctrl | om of every rank by rank
    unsigned long long push_seq = 0;            // barrier sequence number (the same on every rank: lock-step call sequences)
    int64_t n_push_gens = 0;
    // sparse exchange (world > 1, outside CR adaptation): only accepted rows travel, in fixed-capacity packed blocks;
    // a chunk whose capacity was exceeded is rolled back to its checkpoint and replayed with the dense all-gather
    bool sparse_enabled = false;
    // replay exchange (the default for world > 1 outside CR adaptation): owners publish one accept byte per update, every
    // other rank recomputes the accepted proposals into its replica (phase_replay_kernel)
    bool replay_enabled = false;
    bool replay_active = false;   // the generation being prepared writes accept bytes
    bool push_active = false;     // the generation being prepared pushes its accepted rows into the other ranks' replicas
    uint8_t* accbits_all = nullptr;   // [N] accept bytes by global chain id; this rank's block at rank * n_local
    int64_t n_replay_gens = 0;
    bool sparse_active = false;   // the generation being prepared packs its accepted rows
    uint32_t xnsub = 1;           // sub-blocks per rank (a counter each; local chain li packs into sub-block li % xnsub)
    uint32_t xcap = 0, xcap_max = 0;   // capacity of a sub-block (rows per half generation, even) and its ceiling
    double* PK = nullptr;         // packed blocks: rank r at r * xnsub * xstride(), sub-block = [count | ids(cap) | rows(cap * ld)]
    uint32_t xstride() const { return 2u + xcap * (ld + 1u); }
    uint32_t* xstat = nullptr;    // [0] overflow flag, [1] largest count seen
    double* ckpt_G = nullptr;
    double* ckpt_ll = nullptr;
    uint32_t* ckpt_acc = nullptr;
    unsigned long long* ckpt_counters = nullptr;
    int64_t n_sparse_chunks = 0, n_sparse_replays = 0;
    // direct mode: the generation loop's kernels go through the library's own AQL queue (aql_queue.h) instead of the HIP stream.
    // dq_active: work may be in flight on that queue -- every entry point that uses the stream or reads device memory drains
    // it first (check_handle); run_generations waits for the stream before it enters direct mode.
    bpm::DirectQueue* dq = nullptr;
    bool dq_private = false;          // a queue of this sampler's own (rank of a local group under BPM_TEST_PATHS=groupqueues)
    bool dq_active = false;
    bool dq_enabled = true;           // bpm_set_launch_path
    bool shape_needs_scratch = false; // 1024 < d <= 2048 (16 coordinate pairs per lane): the update kernels spill to scratch memory, which the HIP
                                      // runtime provisions for ITS queues -- these samplers launch on the stream
    bool coherent = false;            // state buffers live in cached-coherent device memory (state_mem)
    int dq_fence = bpm::DirectQueue::FENCED;   // fences of the update-kernel packets (run_generations)
    bool timed_direct = false;        // the last bpm_step_timed was timed by the queue's dispatch time stamps
    // run state
    bpm_run_opts_t opts{};
    bool run_open = false;
    int64_t k_gen = 0, t_abs = 0;
    int phase = 0;               // host-callback: next half generation to propose (0/1)
    int64_t phase_a_updates = 0; // host-callback: local chains already updated in an open generation
    bool proposed = false;
    bool state_set = false;
    // convergence diagnostics (diagnostics.h, bpm_diag_*): per-half-chain means and M2 of the window of the last bpm_diag_split_moments
    // ([2][n_local][ld] each), which bpm_diag_autocov centres with; valid while the history is what that call read (dg_seen)
    double* dg_mean = nullptr;
    double* dg_m2 = nullptr;
    double* dg_out = nullptr;       // [max(3, DIAG_T) ld]: the aggregates of the split pass, then one block of lag sums
    double* dg_part = nullptr;      // per-workgroup partials of diag_autocov_kernel
    size_t dg_part_cap = 0;
    HistorySnapshot dg_seen;
    int64_t dg_g0 = 0, dg_g1 = 0, dg_n = 0;
    uint64_t hist_epoch = 0;        // bumped whenever the history is replaced (reset_history, bpm_set_history); generations bump t_abs
    // posterior quantiles (quantiles.h, bpm_quantile_*): the window [qs_lo, qs_hi) of local super-chain rows fixed by the last
    // bpm_quantile_begin, valid while the history is what that call saw (qs_seen); qs_buf holds one histogram request
    // (histograms and NaN counts out, prefixes, coordinates and tiles in), qs_cap bytes
    unsigned char* qs_buf = nullptr;
    size_t qs_cap = 0;
    HistorySnapshot qs_seen;
    uint64_t qs_lo = 0, qs_hi = 0;
    // posterior histograms (histograms.h, bpm_hist_*): the window fixed by the last bpm_hist_range, valid while the history is what that
    // call saw (hs_seen); every device buffer of these calls is temporary
    HistorySnapshot hs_seen;
    uint64_t hs_lo = 0, hs_hi = 0;
    // trace summaries (traces.h, bpm_trace_*): the generations [tr_g0, tr_g1) and the bin width of the last bpm_trace_bins, valid while the
    // history is what that call saw (tr_seen); every device buffer of these calls is temporary
    HistorySnapshot tr_seen;
    int64_t tr_g0 = 0, tr_g1 = 0, tr_every = 1;
    double* om = nullptr;        // outlier check: world x [omega (n_local) | ln_like (n_local)], all-gathered in place
    double* sel = nullptr;       // outlier check: [0..3] order statistics around Q1 / Q3, [4] first argmax of omega
    unsigned char* sel_state = nullptr;   // radix-select state between the passes (SelState)
    bool outlier_due = false;    // set by finish_generation, served by the group driver (all ranks take part)
    // per-generation cache (host-callback path keeps it between propose and commit)
    PhaseArgs cur_args[2];
    // ... and beside it what prepare_generation chose for the two update launches: the kernel flavour (kernels.h: Flavour) and who launches it
    // (the shipped target's table entry, or the run-time module's launcher) -- launch_update launches exactly this
    int cur_hot[2] = {0, 0};
    FusedLaunch cur_launch = nullptr;
    int64_t n_by_flavour[N_FLAVOURS] = {};      // update launches of this handle by flavour, never reset (bpm_debug_flavour_counts)
    // several chains per wavefront + device target (kernels.h: lean_scalars): the update kernels neither read nor write the ln-like cache `ll`
    // (they re-evaluate it from the own row); ll_stale says that generations have run since it was last evaluated -- refresh_ll brings it up
    // to date for whoever reads it (bpm_get_loglike, the outlier check)
    bool lean = false, ll_stale = false;
    bool gen_adapt_on = false;
    bool gen_cr_reduce = false;       // this generation's (delta, cr) slots are reduced (adaptation on AND the gate of dream.py:123 open)
};


static FusedLaunch pick_fused(const bpm_sampler* s) {
    const int v = s->cfg.algo != BPM_ALGO_DREAM ? 0 : (s->cfg.del_pairs == 3 ? 1 : 2);
    switch (s->cfg.target_id) {
        case BPM_TARGET_GAUSS_EQUICORR: return g_fused_gauss[v][s->shape.idx];
        case BPM_TARGET_MIXTURE_PAIRS: return g_fused_mixture[v][s->shape.idx];
        case BPM_TARGET_BANANA_2D: return g_fused_banana[v];
        default: return nullptr;
    }
}
static void launch_user_fused(const PhaseArgs& a, int flavour, hipStream_t st);      // (the run-time module's launcher: below, beside run_generations)
// One update launch of the generation prepare_generation laid out: the argument block, the flavour and the launcher it chose
static inline void launch_update(bpm_sampler* s, int ph) {
    const int f = s->cur_hot[ph];
    ++s->n_by_flavour[f];
    s->cur_launch(s->cur_args[ph], f, s->stream);
}

// leave direct mode: everything dispatched on the library's own queue has finished and is visible to the HIP stream and the host
static int leave_direct(bpm_sampler* s) {
    if (!s->dq_active) return 0;
    s->dq_active = false;
    if (s->dq && s->dq->drain() != 0) return fail("direct AQL queue: " + s->dq->why());
    return 0;
}
static int check_handle(bpm_handle_t h) {
    if (!h) return fail("null handle");
    return leave_direct(h);
}
// A piece of HIP-stream work in the middle of a direct-mode generation loop: queue drained before, stream drained after.
struct StreamSection {
    bpm_sampler* s;
    bool was;
    int rc;
    explicit StreamSection(bpm_sampler* s_);
    int end();
};
static int check_handle_keep_direct(bpm_handle_t h) {      // (bpm_step and friends: consecutive calls stay on the queue)
    if (!h) return fail("null handle");
    return 0;
}
StreamSection::StreamSection(bpm_sampler* s_) : s(s_), was(s_->dq_active && g_disp.dq != nullptr), rc(0) {
    if (was) { s->dq->flush(); rc = s->dq->drain() != 0 ? fail("direct AQL queue: " + s->dq->why()) : 0; }
}
int StreamSection::end() {
    if (!was) return 0;
    CK(wait_stream(s->stream));
    g_disp.mark_acquire(true);
    return 0;
}



static int set_device(bpm_sampler* s) {
    HIPCK(hipSetDevice(s->cfg.device));
    return 0;
}

// Buffers that one update kernel writes and the next one reads (state matrix, ln-like cache, accept counters, Welford moments): ordinary
// device memory, or -- coherent == true, ONLY in the experiment build -DBPM_EXPERIMENT_COHERENT -- the GPU's EXTENDED-SCOPE FINE-GRAINED pool
// (hipDeviceMallocUncached on this runtime): local HBM mapped with the cached-coherent memory type, i.e. the XCDs' L2s stay coherent on
// these lines by themselves (tools/micro/aql_direct.cpp: a dependent chain of kernels is correct on it with NO release fence between
// the dispatches, wrong on hipMalloc memory).  Gathers from it cost 1-5 % more than from ordinary device memory.
static MemKind state_mem(bool coherent) {
#ifdef BPM_EXPERIMENT_COHERENT
    if (coherent) return MEM_UNCACHED;
#endif
    (void)coherent;
    return MEM_DEVICE;
}

// Does memory of state_mem(true) really stay coherent across the XCDs without a release fence?  What hipDeviceMallocUncached maps
// to is the runtime's choice (hsa_amd_pointer_info reports the same flags for it as for plain fine-grained memory, which is NOT
// coherent that way), so the property itself is tested once per device: 48 dependent dispatches with acquire-only packets hand
// every block of a 2 MB buffer from workgroup to workgroup; ordinary memory fails this in every element (tools/micro/aql_direct.cpp).
// -> number of wrong elements (0 = every launch saw its predecessor's writes), -1 = the probe could not run
#if defined(BPM_TEST_HOOKS) || defined(BPM_EXPERIMENT_COHERENT)
static long long coherence_probe(bpm::DirectQueue* dq, bool coherent_alloc) {
    constexpr uint32_t NB = 4096, L = 48;
    DevTemp<double> xb(state_mem(coherent_alloc));
    long long wrong = -1;
    const bpm::DqKernel* k = dq->kernel(reinterpret_cast<const void*>(coherence_probe_kernel));
    if (!dq->set_fence_kernel(reinterpret_cast<const void*>(queue_fence_kernel))) k = nullptr;      // (drain() behind release-less packets)
    if (k && xb.alloc((size_t)NB * WAVE) == 0) {
        double* const x = xb.p;
        std::vector<double> h((size_t)NB * WAVE);
        bool run = hipMemset(x, 0, h.size() * sizeof(double)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        for (uint32_t i = 0; i < L && run; ++i) {
            struct { double* x; uint32_t nb, shift; } a{x, NB, 7u * i};
            run = dq->launch(*k, NB, 1, WAVE, &a, sizeof(a), i == 0 ? bpm::DirectQueue::FENCED : bpm::DirectQueue::ACQUIRE) == 0;
        }
        run = run && dq->drain() == 0 && hipMemcpy(h.data(), x, h.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
        if (run) {
            wrong = 0;
            for (double v : h) wrong += v != (double)L;
        }
        (void)hipGetLastError();
    }
    return wrong;
}
#endif
#ifdef BPM_EXPERIMENT_COHERENT
static bool state_memory_is_coherent(bpm::DirectQueue* dq, int device) {
    static std::mutex mu;
    static std::map<int, bool> known;
    std::lock_guard<std::mutex> lk(mu);
    auto it = known.find(device);
    if (it != known.end()) return it->second;
    const bool ok = coherence_probe(dq, true) == 0;
    known[device] = ok;
    return ok;
}
#endif

// ---- thinned histories: the three questions everything below asks -------------------------------------------------------------------
// stored rows of a history of `rows_logical` logical rows (row 0 = the initial state)
static inline int64_t stored_rows_of(const bpm_sampler* s, int64_t rows_logical) {
    return rows_logical < 1 ? 0 : (rows_logical - 1) / s->hist_stride + 1;
}
// is the history resident: one stored row for every logical row that is a multiple of the stride
static inline bool history_resident(const bpm_sampler* s) {
    return s->cfg.keep_history && s->hist_rows == stored_rows_of(s, s->rows_logical);
}
// is the last stored row the current state (it is not after a generation that was not appended)
static inline bool last_row_is_state(const bpm_sampler* s) {
    return s->hist_rows >= 1 && s->hist_rows == stored_rows_of(s, s->rows_logical) && (s->rows_logical - 1) % s->hist_stride == 0;
}
// does the generation that produces logical row rows_logical append
static inline bool generation_appends(const bpm_sampler* s) {
    return s->cfg.keep_history && (s->hist_stride == 1 || s->rows_logical % s->hist_stride == 0);      // (stride 1: no division in the generation loop)
}
// the stored rows after n_gens more generations: what a step call reserves
static inline int64_t stored_rows_after(const bpm_sampler* s, int64_t n_gens) {
    return s->hist_rows + (stored_rows_of(s, s->rows_logical + std::max<int64_t>(n_gens, 0)) - stored_rows_of(s, s->rows_logical));
}

// The history's growth rule, stated once: the rows ensure_history(s, rows) allocates (0: it fits) ...
static int64_t history_growth(const bpm_sampler* s, int64_t rows) {
    if (!s->cfg.keep_history) rows = std::min<int64_t>(rows, 1);
    return rows <= s->hist_cap ? 0 : std::max<int64_t>(rows, s->hist_cap + s->hist_cap / 2);
}
// ... and the same in bytes, for a caller that sizes its own scratch first: `what` ("derived", "ranked") names the history in the refusal
static int history_growth_bytes(const bpm_sampler* s, int64_t rows, const std::string& who, const char* what, size_t mem_free, uint64_t* need) {
    const uint64_t cap = (uint64_t)history_growth(s, rows);
    *need = cap * s->n_local * ((uint64_t)s->ld + 1u) * sizeof(double);
    if (*need > mem_free)
        return fail(who + ": the " + what + " history of " + std::to_string((long long)cap) + " generations x " + std::to_string(s->n_local) + " chains x (" +
                    std::to_string(s->ld) + " + 1 ln-like) doubles needs " + std::to_string((unsigned long long)(*need >> 20)) + " MiB of device memory; " +
                    std::to_string(mem_free >> 20) + " MiB are free");
    return 0;
}

static int ensure_history(bpm_sampler* s, int64_t rows, bool exact = false) {      // (exact: room for `rows` and no more, where the growth rule's would not fit)
    int64_t cap = history_growth(s, rows);
    if (cap == 0) return 0;
    if (exact) cap = s->cfg.keep_history ? rows : std::min<int64_t>(rows, 1);
    const bool was_direct = s->dq_active;
    CK(leave_direct(s));              // (kernels in flight on the library's own queue still write the old buffers)
    const size_t row_d = (size_t)s->n_local * s->ld;
    DevTemp<double> nh, nl;
    CK(nh.alloc((size_t)cap * row_d));
    CK(nl.alloc((size_t)cap * s->n_local));
    if (s->hist_rows > 0) {
        HIPCK(hipMemcpyAsync(nh.p, s->hist, (size_t)s->hist_rows * row_d * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        HIPCK(hipMemcpyAsync(nl.p, s->llhist, (size_t)s->hist_rows * s->n_local * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    }
    HIPCK(hipStreamSynchronize(s->stream));
    s->mem.replace(&s->hist, nh);
    s->mem.replace(&s->llhist, nl);
    s->hist_cap = cap;
    s->hist_tag.resize((size_t)cap, -1);
    s->dq_active = was_direct && g_disp.dq != nullptr;      // (inside a direct-mode generation: the stream is idle again, go on)
    return 0;
}

// A reservation somebody asked for (bpm_reserve_history, the head of a step call): the growth is checked against the free memory BEFORE anything
// is allocated -- the regrow copy needs the old and the new buffer at once -- and the refusal names the ways out.  The handle stays as it was.
static int reserve_history(bpm_sampler* s, int64_t rows, const char* who) {
    if (history_growth(s, rows) == 0) return 0;
    size_t mem_free = 0, mem_total = 0;
    uint64_t need = 0;
    HIPCK(hipMemGetInfo(&mem_free, &mem_total));
    if (history_growth_bytes(s, rows, who, "chain", mem_free, &need) == 0) return ensure_history(s, rows);
    // the growth rule's half again on top does not fit: the rows asked for, exactly, before refusing (the message then states what they need)
    const uint64_t exact = (uint64_t)rows * s->n_local * ((uint64_t)s->ld + 1u) * sizeof(double);
    if (exact <= mem_free) return ensure_history(s, rows, true);
    return fail(std::string(who) + ": the chain history of " + std::to_string((long long)rows) + " generations x " + std::to_string(s->n_local) + " chains x (" +
                std::to_string(s->ld) + " + 1 ln-like) doubles needs " + std::to_string((unsigned long long)(exact >> 20)) + " MiB of device memory; " +
                std::to_string(mem_free >> 20) + " MiB are free (the old rows stay allocated while they are copied); thin the history (thin=k at construction, "
                "thin_history / bpm_thin_history on a handle that has one) or run with keep_history=False and running_moments=True");
}

// ln_like of n rows (ld doubles apart) by the sampler's shipped target, on its stream; false: a host-callback target has no kernel of its own
static bool launch_eval_target(bpm_sampler* s, const double* X, uint32_t n, double* out) {
    switch (s->cfg.target_id) {
        case BPM_TARGET_GAUSS_EQUICORR: g_eval_gauss[s->shape.idx](X, n, s->ld, s->dim, s->tparams, out, s->stream); return true;
        case BPM_TARGET_MIXTURE_PAIRS: g_eval_mixture[s->shape.idx](X, n, s->ld, s->dim, s->tparams, out, s->stream); return true;
        case BPM_TARGET_BANANA_2D: launch_eval<TARGET_BANANA, 1, 2>(X, n, s->ld, s->dim, s->tparams, out, s->stream); return true;
        default: return false;
    }
}

static int eval_local_ll(bpm_sampler* s) {
    // ln_like of the local chains' current state into the cache (device targets only)
    if (!launch_eval_target(s, s->G + (uint64_t)s->rank * s->L.blk, s->n_local, s->ll)) return 0;      // host callback: caller supplies values via bpm_set_loglike
    HIPCK(hipGetLastError());
    return 0;
}

// the ln-like cache of the local chains, current again (stream work: the caller has drained the library's own queue)
static int refresh_ll(bpm_sampler* s) {
    if (!s->ll_stale) return 0;
    CK(eval_local_ll(s));
    s->ll_stale = false;
    return 0;
}

// History rows [r0, r1) into chain order (see bpm_sampler::hist_by_pos).  On the sampler's stream: the caller has drained the library's
// own queue (check_handle / StreamSection).
static int normalize_history(bpm_sampler* s, int64_t r0, int64_t r1) {
    if (!s->hist_by_pos) return 0;
    r0 = std::max<int64_t>(r0, 0);
    r1 = std::min<int64_t>(r1, std::min<int64_t>(s->hist_rows, (int64_t)s->hist_tag.size()));
    const size_t row_d = (size_t)s->n_local * s->ld;
    const uint64_t n = (uint64_t)s->n_local * (s->ld / 2u);
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t tag = s->hist_tag[(size_t)r];
        if (tag < 0) continue;
        const PermKey key = make_perm_key(s->cfg.seed, (uint64_t)(tag >> 2), s->N, (tag & 1) != 0);
        const bool ll_by_chain = (tag & 2) != 0;
        double* row = s->hist + (uint64_t)r * row_d;
        double* llrow = s->llhist + (uint64_t)r * s->n_local;
        hipLaunchKernelGGL(hist_unpermute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, key, s->N, s->ld, (const double*)row,
                           ll_by_chain ? (const double*)nullptr : (const double*)llrow, s->hist_tmp, s->hist_tmp + row_d);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(row, s->hist_tmp, row_d * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        if (!ll_by_chain) HIPCK(hipMemcpyAsync(llrow, s->hist_tmp + row_d, (size_t)s->n_local * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        s->hist_tag[(size_t)r] = -1;
    }
    return 0;
}

// ---- shared by the statistics of the history (bpm_reduce_moments ... bpm_trace_chains) -------------------------------------------------
static int require_resident_history(const bpm_sampler* s, const char* who) {
    if (!history_resident(s))
        return fail(std::string(who) + ": needs keep_history=True (a resident history of every generation)");
    return 0;
}

// param_est's selection (demc.py:235-248): this rank's rows [lo, hi), lo <= hi, of the super chain (row g*N + i = chain i at generation g)
// at or after n_burn (negative: 0).  A partial first generation is counted by chain index, so that row is brought into chain order first.
// (the bounds alone, nothing launched: *partial_row = the history row of a partial first generation, -1 if there is none)
static void super_chain_bounds(const bpm_sampler* s, int64_t n_burn, uint64_t* lo, uint64_t* hi, int64_t* partial_row) {
    if (n_burn < 0) n_burn = 0;
    const int64_t g0 = n_burn / s->N;
    int64_t first = n_burn % s->N - (int64_t)s->lo;      // first local chain of generation g0 that counts
    first = std::max<int64_t>(0, std::min<int64_t>(first, s->n_local));
    *partial_row = first != 0 && g0 < s->hist_rows ? g0 : -1;
    *hi = (uint64_t)s->hist_rows * s->n_local;
    *lo = std::min(*hi, (uint64_t)std::min<int64_t>(g0, s->hist_rows) * s->n_local + (g0 < s->hist_rows ? (uint64_t)first : 0));
}
static int super_chain_window(bpm_sampler* s, int64_t n_burn, uint64_t* lo, uint64_t* hi) {
    int64_t partial_row = -1;
    super_chain_bounds(s, n_burn, lo, hi, &partial_row);
    if (partial_row >= 0) CK(normalize_history(s, partial_row, partial_row + 1));
    return 0;
}

// ---- the one frame of a statistic of an installed function over the window (bpm_derive, bpm_pointwise, bpm_loo) ----------------------------
// This call's window: this rank's super-chain rows [lo, hi) at or after n_burn
struct RowWindow { uint64_t lo = 0, hi = 0, rows = 0; };
// Every refusal that comes before the window, in their order: the handle, the device, a null argument, n_burn, installed() -- 0, or the caller's
// fail() when nothing is installed -- and the resident history; then the window itself.
template <class Installed>
static int open_window(bpm_handle_t s, const std::string& who, bool null_argument, int64_t n_burn, Installed installed, RowWindow& w) {
    CK(check_handle(s));
    CK(set_device(s));
    if (null_argument) return fail(who + ": null argument");
    if (n_burn < 0) return fail(who + ": n_burn must be >= 0 (got " + std::to_string((long long)n_burn) + ")");
    CK(installed());
    CK(require_resident_history(s, who.c_str()));
    CK(super_chain_window(s, n_burn, &w.lo, &w.hi));
    w.rows = w.hi - w.lo;
    return 0;
}
// The optional `values` return of a window, "<rows> rows x <per_row> <noun>" ...
static std::string values_shape(const RowWindow& w, uint64_t per_row, const char* noun) {
    return std::to_string((unsigned long long)w.rows) + " rows x " + std::to_string((unsigned long long)per_row) + " " + noun;
}
// ... can be returned, into the caller's values_cap doubles (values == nullptr: not asked for)
static int check_values(const std::string& who, const double* values, int64_t values_cap, const RowWindow& w, uint64_t per_row, const char* noun) {
    const std::string n_val = std::to_string((unsigned long long)(w.rows * per_row));
    if (values && w.rows * per_row >= (1ull << 31))
        return fail(who + ": the values of " + values_shape(w, per_row, noun) + " are " + n_val + " elements; fewer than 2^31 per rank can be returned");
    if (values && (values_cap < 0 || (uint64_t)values_cap < w.rows * per_row))
        return fail(who + ": values holds " + std::to_string((long long)values_cap) + " doubles; the window needs " + n_val);
    return 0;
}
// One launch over the window's rows, brought into chain order first, into records of `fields` x per_row doubles: [part records | folded records] in
// one buffer (with one part the part records are the folded ones).  launch(part records, n_rec, values on the device or null) fills the part records,
// fold(part records, folded) enqueues the fold kernel -- only with parts > 1.  The folded records come back in out[fields * per_row], the values in `values`; waits.
template <class Launch, class Fold>
static int window_records(bpm_sampler* s, const std::string& who, const RowWindow& w, uint64_t parts, const char* part_noun, size_t fields, uint64_t per_row,
                          const char* noun, double* values, Launch launch, Fold fold, double* out) {
    const uint64_t n_rec = parts * per_row, n_val = w.rows * per_row;
    const size_t o_fold = fields * n_rec;
    CK(normalize_history(s, (int64_t)(w.lo / s->n_local), s->hist_rows));
    DevTemp<double> b, v;
    CK(b.alloc(o_fold + (parts > 1 ? fields * per_row : 0), who.c_str(), "the part records of " + std::to_string((unsigned long long)parts) + " " + part_noun));
    if (values) CK(v.alloc((size_t)n_val, who.c_str(), "the values of " + values_shape(w, per_row, noun)));
    HIPCK(launch(b.p, n_rec, v.p));
    if (parts > 1) { fold((const double*)b.p, b.p + o_fold); HIPCK(hipGetLastError()); }
    HIPCK(hipMemcpyAsync(out, b.p + (parts > 1 ? o_fold : 0), fields * per_row * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (values) HIPCK(hipMemcpyAsync(values, v.p, (size_t)n_val * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

void HistorySnapshot::take(const bpm_sampler* s) {
    epoch = s->hist_epoch; tabs = s->t_abs; rows = s->hist_rows;
    valid = true;
}
int HistorySnapshot::check(const bpm_sampler* s, const char* who, const char* first_call) const {
    if (!valid) return fail(std::string(who) + ": call " + first_call + " first");
    if (epoch != s->hist_epoch || tabs != s->t_abs || rows != s->hist_rows || !history_resident(s))
        return fail(std::string(who) + ": the history changed since " + first_call + " (a step, set_history or set_state); call it again");
    return 0;
}

// How a buffer the sampler keeps between calls grows: the new one, n elements, belongs to this call until it holds the first n_kept of the old
// one and (wait) the stream is done with the old one; only then does it take the old one's place in the registry, and the old one goes.  An
// error on the way leaves the sampler as it was.
template <class T>
static int regrow(bpm_sampler* s, T** p, size_t n, size_t n_kept, bool wait) {
    DevTemp<T> fresh;
    CK(fresh.alloc(n));
    if (n_kept > 0) HIPCK(hipMemcpyAsync(fresh.p, *p, n_kept * sizeof(T), hipMemcpyDeviceToDevice, s->stream));
    if (wait) HIPCK(hipStreamSynchronize(s->stream));
    s->mem.replace(p, fresh);
    return 0;
}
// ... to `need` elements when it is smaller, keeping nothing
template <class T>
static int grow_device(bpm_sampler* s, T** p, size_t* cap, size_t need) {
    if (need <= *cap) return 0;
    CK(regrow(s, p, need, 0, *p != nullptr));
    *cap = need;
    return 0;
}

// workgroups along the rows: about 2048 in all (four resident per CU), each at least 4 sweeps of `rows_per_sweep`, none with 2^31 rows or
// more (a workgroup's uint32 counts stay below 2^31)
static int rows_grid(uint64_t rows, uint64_t n_tiles, uint64_t rows_per_sweep, const char* who, uint64_t* nby_out) {
    uint64_t nby = std::max<uint64_t>(1, 2048 / n_tiles);
    nby = std::min<uint64_t>(nby, (rows + 4 * rows_per_sweep - 1) / (4 * rows_per_sweep));
    nby = std::max<uint64_t>(nby, (rows >> 31) + 1);
    if (nby > 65535) return fail(std::string(who) + ": window too large");
    *nby_out = nby;
    return 0;
}

// n coordinates as the uint32 the kernels read
static void stage_dims(unsigned char* dst, const int32_t* dims, size_t n) {
    for (size_t j = 0; j < n; ++j) {
        const uint32_t k = (uint32_t)dims[j];
        std::memcpy(dst + 4 * j, &k, 4);
    }
}

// the coordinates dims[0 .. n_dims) exist; each one's bins + 1 edges are finite and non-decreasing
static int check_dims_edges(const bpm_sampler* s, const char* who, uint32_t n_dims, const int32_t* dims, uint32_t bins, const double* edges) {
    for (uint32_t j = 0; j < n_dims; ++j) {
        if (dims[j] < 0 || (uint32_t)dims[j] >= s->dim) return fail(std::string(who) + ": coordinate out of range");
        const double* e = edges + (size_t)j * (bins + 1);
        for (uint32_t i = 0; i <= bins; ++i)
            if (!std::isfinite(e[i]) || (i > 0 && e[i] < e[i - 1])) return fail(std::string(who) + ": edges must be finite and non-decreasing");
    }
    return 0;
}

// ---- running population sums (cfg.running_moments) -------------------------------------------------------------------------
static int ensure_gen_sums(bpm_sampler* s, int64_t rows) {
    if (!s->cfg.running_moments || rows <= s->gen_sums_cap) return 0;
    const bool was_direct = s->dq_active;
    CK(leave_direct(s));
    const int64_t cap = std::max<int64_t>(std::max<int64_t>(rows, 1024), s->gen_sums_cap + s->gen_sums_cap / 2);
    const size_t n_kept = s->gen_sums && s->rows_logical > 0 ? (size_t)std::min<int64_t>(s->rows_logical, s->gen_sums_cap) * 2 * s->ld : 0;
    CK(regrow(s, &s->gen_sums, (size_t)cap * 2 * s->ld, n_kept, true));
    s->gen_sums_cap = cap;
    s->dq_active = was_direct && g_disp.dq != nullptr;
    return 0;
}
// the sums of history row `row` from this rank's block of the state matrix as it stands (two dispatches: per-block partial sums, a
// fixed-order fold -- the kernels of bpm_reduce_moments, hence the same bits for the same rows)
static int push_gen_sums(bpm_sampler* s, int64_t row, const double* src = nullptr) {
    if (!s->cfg.running_moments) return 0;
    const double* Xl = src ? src : s->G + (uint64_t)s->rank * s->L.blk;
    double* out = s->gen_sums + (size_t)row * 2 * s->ld;
    // (on the queue: reads rows that update kernels wrote, possibly with agent-scope stores behind release-less packets: acquire; writes what only
    // bpm_reduce_moments reads, behind a drain: plain stores, release left to the drain's fence kernel)
    CK(launch_side(s->stream, moments_partial_kernel, "running-moment kernels", dim3(s->gs_nb), MOM_THREADS, bpm::DirectQueue::FENCED, Then::KEEP, Xl, 0, s->n_local, s->ld, s->gs_shift, s->gs_part));
    return launch_side(s->stream, moments_final_kernel, "running-moment kernels", dim3(s->ld), MOM_THREADS, bpm::DirectQueue::FENCED, Then::ACQUIRE, s->gs_part, s->gs_nb, s->ld, out);
}

// after the state matrix was (re)initialised: history := [state], moments reset
static int reset_history(bpm_sampler* s) {
    s->hist_epoch += 1;
    CK(eval_local_ll(s));
    s->ll_stale = false;
    s->hist_rows = 0;
    s->rows_logical = 1;
    s->w_rows = 0;
    CK(ensure_history(s, 1));
    const size_t row_d = (size_t)s->n_local * s->ld;
    HIPCK(hipMemcpyAsync(s->hist, s->G + (uint64_t)s->rank * s->L.blk, row_d * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    HIPCK(hipMemcpyAsync(s->llhist, s->ll, (size_t)s->n_local * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (!s->hist_tag.empty()) s->hist_tag[0] = -1;
    s->hist_rows = 1;
    // Welford over the single row: mean = row, m2 = 0
    // (one record per chain: [mean (ld) | m2 (ld)])
    HIPCK(hipMemsetAsync(s->w_mean, 0, 2 * row_d * sizeof(double), s->stream));
    HIPCK(hipMemcpy2DAsync(s->w_mean, (size_t)2 * s->ld * sizeof(double), s->hist, (size_t)s->ld * sizeof(double), (size_t)s->ld * sizeof(double), s->n_local,
                           hipMemcpyDeviceToDevice, s->stream));
    s->w_rows = 1;
    if (s->cfg.running_moments) {      // shift := chain 0's state; sums of row 0
        HIPCK(hipMemcpyAsync(s->gs_shift, s->G, s->ld * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        CK(ensure_gen_sums(s, 1));
        CK(push_gen_sums(s, 0));
    }
    s->state_set = true;
    s->phase = 0;
    s->proposed = false;
    return 0;
}

// BPM_TEST_PATHS=hosttiming (diagnostic): host nanoseconds spent preparing generations and inside the launch calls, printed by bpm_destroy
static bool g_host_timing = test_path("hosttiming");
static long long g_ns_prepare = 0, g_ns_launch = 0, g_n_launch = 0;
static std::vector<long long> g_launch_log;       // (start, end) of every launch call of the current bpm_step_timed
static inline long long now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The decision bpm_destroy takes about the sampler's device buffers, as a pure function: 1 = free them, 0 = leak them.  Buffers are freed unless
// the queue that may still run kernels on them failed AND could not be quiesced.  (CPU-tested through the test variant: bpm_debug_destroy_plan.)
static int destroy_plan(int queue_failed, int quiesced) { return (queue_failed != 0 && quiesced == 0) ? 0 : 1; }
extern "C" const char* bpm_last_error(void) { return g_err.c_str(); }
extern "C" int bpm_abi_version(void) { return BPM_ABI_VERSION; }
// Which sources is this binary?  The Makefile bakes in the first 16 hex digits of the SHA-256 over sampler.hip, the kernel headers, both C headers and
// the Makefile itself (ID_SRCS, in that order); bipymc_amd/_lib.py recomputes it from the tree and refuses a library built from other sources.
#ifndef BPM_BUILD_ID
#define BPM_BUILD_ID "unknown"
#endif
extern "C" const char* bpm_build_id(void) { return BPM_BUILD_ID; }
extern "C" int bpm_device_count(int32_t* out) {
    if (!out) return fail("bpm_device_count: null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *out = n;
    return 0;
}

extern "C" int bpm_get_unique_id(char out[BPM_UID_BYTES]) {
    CK(load_rccl());
    ncclUniqueId id;
    NCCLCK(g_rccl.GetUniqueId(&id));
    static_assert(sizeof(id) == BPM_UID_BYTES, "uid size");
    std::memcpy(out, &id, BPM_UID_BYTES);
    return 0;
}

extern "C" int bpm_destroy(bpm_handle_t s) {
    if (!s) return 0;
    if (g_host_timing && g_n_launch > 0) {
        fprintf(stderr, "[bpm host timing] %lld launches: %.2f us per launch call, %.2f us per generation in prepare_generation\n", g_n_launch,
                g_ns_launch * 1e-3 / g_n_launch, g_ns_prepare * 2e-3 / g_n_launch);
        g_ns_prepare = g_ns_launch = g_n_launch = 0;
    }
    (void)hipSetDevice(s->cfg.device);
    // What the library's own queue still holds must be finished -- or aborted -- before the buffers its kernels use are freed: the raw
    // HSA queue is invisible to hipStreamSynchronize and hipFree.  After a drain that ran into its time limit (a tool stalling the
    // queue: DESIGN.md section 5 "Dispatch") the kernels may be slow, not dead; DirectQueue::quiesce then inactivates the queue, and if
    // even that is refused the device buffers are deliberately LEAKED and the call reports it.
    const int drained = leave_direct(s);
    const bool queue_failed = s->dq != nullptr && (drained != 0 || s->dq->failed());
    const bool quiet = !queue_failed || s->dq->quiesce();
    const bool free_buffers = destroy_plan(queue_failed ? 1 : 0, quiet ? 1 : 0) == 1;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    // Push exchange between processes: the library orders the teardown itself (round 3 relied on the caller's barrier).  Announce "closing" in
    // every peer's control block -- a peer that still waits for this rank then reports it at once instead of sitting out its limit -- and wait,
    // bounded (BPM_PUSH_CLOSE_TIMEOUT_S, default 3), until the peers have announced the same: ranks that end a run together unmap each other's
    // arenas only after ALL of them have left their last kernels.  A peer that is late keeps what it mapped alive through its own mapping.
    // (Ranks of ONE process -- local test groups -- are destroyed one after the other by one host thread: nothing to order, and a peer's
    // control block may be gone already.)
    if (s->push_connected && s->world > 1 && !s->local_group && s->stream && s->tab_all && s->ctrl && free_buffers) {
        static const double cto = getenv("BPM_PUSH_CLOSE_TIMEOUT_S") ? atof(getenv("BPM_PUSH_CLOSE_TIMEOUT_S")) : 3.0;
        hipLaunchKernelGGL(push_close_kernel, dim3(1), dim3(WAVE), 0, s->stream, s->ctrl, (const unsigned long long*)(s->tab_all + MAX_SEG), s->world, s->rank,
                           cto > 0.0 ? 1u : 0u, (unsigned long long)(std::max(0.0, cto) * 1e8));
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s->stream);
    }
    if (s->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(s->comm);
    for (uint32_t p = 0; p < (uint32_t)MAX_SEG; ++p) {
        if (s->peer_opened[p] && s->peer_base[p]) (void)hipIpcCloseMemHandle(s->peer_base[p]);
        if (s->peer_ctrl_opened[p] && s->peer_ctrl_base[p]) (void)hipIpcCloseMemHandle(s->peer_ctrl_base[p]);
    }
    if (!free_buffers) s->mem.forget_all();
    s->mem.free_all();
    for (hipEvent_t e : s->chunk_ev) if (e) (void)hipEventDestroy(e);
    // (the run-time modules and their parameter blocks go the way of the buffers)
    if (free_buffers) { s->like.fused.drop(s->dq); s->like = UserLikelihood(); s->derived = DerivedFunction(); s->pointwise = PointwiseFunction(); }
    else { s->like.leak(); s->derived.leak(); s->pointwise.leak(); }
    for (auto& B : s->tb)
        if (B.built) (void)hipEventDestroy(B.built);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    if (s->dq_private && free_buffers) bpm::DirectQueue::destroy_private(s->dq);
    delete s;
    if (!free_buffers)
        return fail("bpm_destroy: the library's AQL queue failed and could not be quiesced; the sampler's device buffers were leaked "
                    "rather than freed under kernels that may still run");
    return 0;
}

#ifdef BPM_TEST_HOOKS
// ---- test hooks (include/bipymc_hip_test.h; build_variants/libbipymc_test.so only) -----------------------------------------------------
extern "C" int bpm_debug_destroy_plan(int32_t queue_failed, int32_t quiesced) { return destroy_plan(queue_failed, quiesced); }

// Test hook: put the handle's queue into the state a timed-out drain leaves (refuse_quiesce != 0: and make quiesce() fail as if
// hsa_queue_inactivate had been refused).  The queue of this device is then unusable for the rest of the PROCESS -- run in a child process.
extern "C" int bpm_debug_fail_queue(bpm_handle_t s, int32_t refuse_quiesce) {
    if (!s) return fail("null handle");
    if (!s->dq) return fail("bpm_debug_fail_queue: this sampler has no queue of its own");
    s->dq->test_mark_failed(refuse_quiesce != 0);
    return 0;
}

// Test hook: no-op packets on the handle's queue until its next packet takes position `pos` (0 ... 254) of an epoch of 256 packets; *widx = the
// queue's write index afterwards.  (tests/test_gpu_api.py::test_drains_at_every_position_of_the_queues_epochs)
extern "C" int bpm_debug_queue_pad(bpm_handle_t s, int32_t pos, int64_t* widx) {
    if (!s) return fail("null handle");
    if (!s->dq) return fail("bpm_debug_queue_pad: this sampler has no queue of its own");
    if (pos < 0 || pos > 254) return fail("bpm_debug_queue_pad: pos must be 0 ... 254");
    const int64_t w = s->dq->test_pad_to((uint32_t)pos);
    if (w < 0) return fail("bpm_debug_queue_pad: " + s->dq->why());
    if (widx) *widx = w;
    return 0;
}
#endif   // BPM_TEST_HOOKS

extern "C" int bpm_create(const bpm_config_t* cfg, bpm_handle_t* out) {
    if (!cfg || !out) return fail("bpm_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != BPM_ABI_VERSION) return fail("bpm_create: ABI version mismatch");
    if (cfg->algo != BPM_ALGO_DEMC && cfg->algo != BPM_ALGO_DREAM && cfg->algo != BPM_ALGO_DEMC_SYNC) return fail("bpm_create: unknown algo");
    if (cfg->n_chains < 4) return fail("bpm_create: n_chains >= 4 required (samplers.py:249)");
    if (cfg->dim < 1) return fail("bpm_create: dim >= 1 required");
    if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) return fail("bpm_create: bad rank/world_size");
    if (cfg->n_chains % cfg->world_size != 0)
        return fail("bpm_create: n_chains must be divisible by world_size (unequal blocks break Allgather, demc.py:39,93)");
    if (cfg->algo == BPM_ALGO_DREAM) {
        if (cfg->del_pairs < 1 || cfg->del_pairs > MAX_PAIRS) return fail("bpm_create: 1 <= del_pairs <= 10");
        if (cfg->n_cr < 1 || cfg->n_cr > BPM_MAX_CR) return fail("bpm_create: 1 <= n_cr <= 8");
    }
    int ndev = 0;
    HIPCK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail("bpm_create: no HIP device (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail("bpm_create: device ordinal out of range");

    bpm_sampler* s = new bpm_sampler();
    s->cfg = *cfg;
    s->cfg.target_params = nullptr;
    s->cfg.nccl_uid = nullptr;
    s->N = (uint32_t)cfg->n_chains;
    s->dim = (uint32_t)cfg->dim;
    s->ld = (s->dim + 1u) & ~1u;
    s->world = (uint32_t)cfg->world_size;
    s->rank = (uint32_t)cfg->rank;
    s->n_local = s->N / s->world;
    s->lo = s->rank * s->n_local;
    (void)pick_shape(s->ld, s->shape);
    // (the one limit on dim: a coordinate pair's Philox block is addressed by a 16-bit slot, philox.h: SLOT_BITS)
    if (s->dim / 2u + SLOT_DIM0 >= (1u << SLOT_BITS)) { delete s; return fail("bpm_create: dim must stay below 131056 (16-bit Philox slot per coordinate pair)"); }
    s->shape_needs_scratch = false;        // (round 3's 32-coordinates-per-lane shape spilled to scratch memory; the looped kernel replaced it)
    if ((uint64_t)s->N * (s->ld + 2) >= (1ull << 31)) { delete s; return fail("bpm_create: n_chains * (dim + 2) must stay below 2^31 (32-bit device offsets)"); }
    const int tid = cfg->target_id;
    const int np = cfg->n_target_params;
    bool ok = true;
    if (tid == BPM_TARGET_GAUSS_EQUICORR) ok = (np == 4 + (int)s->dim);
    else if (tid == BPM_TARGET_MIXTURE_PAIRS) ok = (np == 16 && s->dim % 2 == 0);
    else if (tid == BPM_TARGET_BANANA_2D) ok = (np == 9 && s->dim == 2);
    else if (tid != BPM_TARGET_HOST_CALLBACK) ok = false;
    if (!ok || (np > 0 && !cfg->target_params)) { delete s; return fail("bpm_create: target id / parameter block / dim mismatch"); }
    if (np > 0) s->tparams_h.assign(cfg->target_params, cfg->target_params + np);
    if (cfg->algo != BPM_ALGO_DREAM) { s->cfg.del_pairs = 1; s->cfg.n_cr = 1; }
    if (cfg->algo == BPM_ALGO_DEMC_SYNC) s->cfg.p_snooker = 0.0;

#define CKD(expr)                                   \
    do {                                            \
        int _r = (expr);                            \
        if (_r != 0) { bpm_destroy(s); return _r; } \
    } while (0)
#define HIPCKD(expr)                                                                             \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            bpm_destroy(s);                                                                      \
            return fail(std::string(#expr) + " failed: " + hipGetErrorString(_e));               \
        }                                                                                        \
    } while (0)
    HIPCKD(hipSetDevice(cfg->device));
    HIPCKD(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    // The per-generation tables are built on the update stream itself, ONE WINDOW AHEAD (on entering window W the build of W + 1 is
    // enqueued in front of W's first update kernel): 16 us per 64 generations at cfg2, and no bpm_step call ever starts with a table
    // build.  (A second stream for the build measured SLOWER on MI355X, 13.7 vs 12.3 us per generation at cfg2:
    // profiles/r02_table_build_modes.txt; removed in round 3.)
    // the library's own AQL queue for the steady state of a single-GPU sampler (aql_queue.h); without it (no large BAR, a runtime
    // without the loader extension, BPM_DIRECT_QUEUE=0) the same kernels are launched on the stream
    // (a host-callback sampler uses it once it has been given a likelihood as HIP source: the update kernel compiled around it, bpm_set_device_likelihood)
    {
        s->dq = bpm::DirectQueue::for_device(cfg->device);
        if (s->dq && s->dq->failed()) s->dq = nullptr;       // (a queue that failed earlier in this process is not adopted: HIP stream launches)
        if (s->dq && !s->dq->kernel(reinterpret_cast<const void*>(perm_table_kernel))) s->dq = nullptr;      // (HIP's copy of the code object not found)
    }
    // The state lives in ordinary device memory; the steady-state packets of the generation loop carry the acquire fence only and the
    // update kernel writes what its successor reads with agent-scope stores (Dispatch::update_fence above).  Without the fence kernel (not
    // found among the loaded code objects): acquire + release on every packet, like a HIP stream; bpm_set_launch_path chooses per handle.
    // The round-2 experiment that kept the state in the GPU's hardware-coherent memory type with acquire-only packets is NOT part of
    // this library: histories came back with older contents in sequences of samplers created and destroyed in one process, cause not
    // found (profiles/r02_coherent_memory_hazard.txt).  It builds only as `make variant NAME=coherent DEFS=-DBPM_EXPERIMENT_COHERENT`.
    {
#ifdef BPM_EXPERIMENT_COHERENT
        const char* c = getenv("BPM_COHERENT_STATE");      // (=2: take the memory type on trust, without the probe)
        s->coherent = s->dq != nullptr && c && atoi(c) != 0 && (atoi(c) == 2 || state_memory_is_coherent(s->dq, cfg->device));
#endif
        const bool fence_kernel = s->dq != nullptr && s->dq->set_fence_kernel(reinterpret_cast<const void*>(queue_fence_kernel));
        s->dq_fence = fence_kernel ? bpm::DirectQueue::ACQUIRE : bpm::DirectQueue::FENCED;
#ifdef BPM_EXPERIMENT_COHERENT
        if (const char* f = getenv("BPM_DQ_FENCE")) if (s->coherent && !strcmp(f, "none")) s->dq_fence = 0;
#endif
    }
    HIPCKD(hipEventCreate(&s->ev0));
    HIPCKD(hipEventCreate(&s->ev1));
    for (auto& B : s->tb) HIPCKD(hipEventCreateWithFlags(&B.built, hipEventDisableTiming));
    s->L.blk = (uint64_t)s->n_local * (s->ld + 2);
    s->L.magic = (uint32_t)((1ull << 32) / s->n_local) + 1u;
    s->L.n_local = s->n_local; s->L.ld = s->ld; s->L.dim = s->dim; s->L.world = s->world;
    const size_t row_d = (size_t)s->n_local * s->ld;
    const bool want_om = cfg->algo == BPM_ALGO_DREAM && cfg->outlier_every > 0;
    if (s->world > 1 && s->world <= (uint32_t)MAX_SEG && cfg->algo != BPM_ALGO_DEMC_SYNC && cfg->target_id != BPM_TARGET_HOST_CALLBACK) {
        // the arena of the push exchange: [G | om | control block], one allocation = one IPC handle
        auto up = [](size_t b) { return (b + 255u) & ~(size_t)255u; };
        const size_t g_bytes = up((size_t)s->world * s->L.blk * sizeof(double));
        const size_t om_bytes = want_om ? up((size_t)s->world * 2 * s->n_local * sizeof(double)) : 0;
        s->off_om = g_bytes; s->off_ctrl = g_bytes + om_bytes;
        s->arena_bytes = s->off_ctrl + up(sizeof(PushCtrl));
        unsigned char* arena = nullptr;
        CKD(s->mem.alloc(&arena, s->arena_bytes));
        s->arena = arena;
        HIPCKD(hipMemsetAsync(s->arena, 0, s->arena_bytes, s->stream));
        s->G = reinterpret_cast<double*>(s->arena);
        if (want_om) s->om = reinterpret_cast<double*>(reinterpret_cast<char*>(s->arena) + s->off_om);
        s->ctrl = reinterpret_cast<PushCtrl*>(reinterpret_cast<char*>(s->arena) + s->off_ctrl);
        {   // The flags are polled INSIDE a kernel while other agents write them: the memory model promises coherence across agents for
            // fine-grained memory only (coarse-grained: at kernel boundaries).  So the control block gets a fine-grained allocation of its own
            // when the runtime gives one that can be exported; else it stays in the arena (ranks sharing one GPU do not need more).
            DevTemp<unsigned char> fg(MEM_FINEGRAINED);
            hipIpcMemHandle_t probe;
            if (!test_path("ctrlarena") && fg.get(up(sizeof(PushCtrl))) == hipSuccess && fg.p &&
                hipMemset(fg.p, 0, up(sizeof(PushCtrl))) == hipSuccess && hipIpcGetMemHandle(&probe, fg.p) == hipSuccess) {
                s->ctrl = reinterpret_cast<PushCtrl*>(s->mem.keep(fg));
                s->ctrl_fine = true;
            } else {
                (void)hipGetLastError();
            }
        }
        CKD(s->mem.alloc(&s->tab_peerG, (size_t)MAX_PEERS));
        CKD(s->mem.alloc(&s->tab_all, (size_t)3 * MAX_SEG));
        HIPCKD(hipMemsetAsync(s->tab_peerG, 0, MAX_PEERS * sizeof(unsigned long long), s->stream));
        HIPCKD(hipMemsetAsync(s->tab_all, 0, 3 * MAX_SEG * sizeof(unsigned long long), s->stream));
    } else {
        CKD(s->mem.alloc(&s->G, (size_t)s->world * s->L.blk, state_mem(s->coherent)));
        HIPCKD(hipMemsetAsync(s->G, 0, (size_t)s->world * s->L.blk * sizeof(double), s->stream));
    }
    s->L.G = s->G;
    CKD(s->mem.alloc(&s->ll, s->n_local, state_mem(s->coherent)));
    CKD(s->mem.alloc(&s->w_mean, 2 * row_d, state_mem(s->coherent)));      // one record per chain: [mean (ld) | m2 (ld)]
    s->w_m2 = s->w_mean + s->ld;
    CKD(s->mem.alloc(&s->tparams, (size_t)np + 2));       // (+2: the wide-row kernels read the Gaussian's 1/sigma as pairs)
    HIPCKD(hipMemsetAsync(s->tparams, 0, ((size_t)np + 2) * sizeof(double), s->stream));
    if (np > 0) HIPCKD(hipMemcpyAsync(s->tparams, s->tparams_h.data(), (size_t)np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    CKD(s->mem.alloc(&s->cr_state_base, 6 * MAX_CR, state_mem(s->coherent)));
    s->cr_state = s->cr_state_base; s->cr_state_alt = s->cr_state_base + 3 * MAX_CR;
    if (cfg->algo == BPM_ALGO_DREAM) {       // the partial sums of the CR reduction (kernels.h)
        const uint32_t n_first = (s->N + 1u) / 2u;
        s->cr_g1 = (uint32_t)cr_g1(s->shape.lpc);
        s->cr_n1 = cr_chunks_of(n_first, s->cr_g1) + cr_chunks_of(s->N - n_first, s->cr_g1);
        const size_t n2 = ((size_t)s->cr_n1 + WAVE - 1) / WAVE;
        CKD(s->mem.alloc(&s->cr_p1, (size_t)4 * MAX_CR * s->cr_n1, state_mem(s->coherent)));
        HIPCKD(hipMemsetAsync(s->cr_p1, 0, (size_t)4 * MAX_CR * s->cr_n1 * sizeof(double), s->stream));
        s->cr_p1_cur = s->cr_p1;
        if (s->cr_n1 > CR_FINAL_MAX)
            for (auto& b : s->cr_p2) { CKD(s->mem.alloc(&b, (size_t)2 * MAX_CR * n2, state_mem(s->coherent))); HIPCKD(hipMemsetAsync(b, 0, (size_t)2 * MAX_CR * n2 * sizeof(double), s->stream)); }
    }
    {
        double init[3 * MAX_CR] = {0};
        for (int m = 0; m < s->cfg.n_cr; ++m) init[m] = 1.0 / s->cfg.n_cr;   // dream.py:114
        HIPCKD(hipMemcpyAsync(s->cr_state, init, sizeof(init), hipMemcpyHostToDevice, s->stream));
        HIPCKD(hipMemcpyAsync(s->cr_state_alt, init, sizeof(init), hipMemcpyHostToDevice, s->stream));
        HIPCKD(hipStreamSynchronize(s->stream));
    }
    // position-ordered history append: one wavefront per chain writes whole 128-byte lines whatever the row's place, nothing to gain there
    // the lean form of the small-d update kernels (kernels.h: lean_scalars) where a launch is transaction bound: from 49152 chains per GPU
    // (cfg3's 65536 and cfg5's 262144 gain 0.6 / 2.6 us per generation, cfg5's per-GPU share of 32768 would lose 0.6)
    // (the banana's kernels have the lean form only: its ln_like is a dozen flops)
    s->lean = s->shape.idx < 3 && tid != BPM_TARGET_HOST_CALLBACK &&
              (tid == BPM_TARGET_BANANA_2D || ((s->n_local >= 49152u || test_path("lean")) && !test_path("nolean")));
    // (a host-callback sampler: used only while the update kernel compiled around its HIP-source likelihood drives it -- prepare_generation asks Dispatch::user_cur;
    // the proposal / commit kernels of the host transports append by chain)
    s->hist_by_pos = s->world == 1 && s->shape.idx < 3 && cfg->keep_history != 0 && cfg->algo != BPM_ALGO_DEMC_SYNC && !test_path("histchain");
    if (s->hist_by_pos) CKD(s->mem.alloc(&s->hist_tmp, (size_t)s->n_local * (s->ld + 1)));
    if (s->cfg.running_moments) {
        s->gs_nb = (uint32_t)std::max<uint32_t>(1u, std::min<uint32_t>(256u, (s->n_local + 63u) / 64u));
        CKD(s->mem.alloc(&s->gs_shift, (size_t)s->ld));
        CKD(s->mem.alloc(&s->gs_part, (size_t)s->gs_nb * 2 * s->ld));
    }
    CKD(s->mem.alloc(&s->counters, 8));      // [2] NaN ratios of this run; [4] outlier resets since creation
    CKD(s->mem.alloc(&s->acc_count, (size_t)s->n_local + ACC_SHARDS, state_mem(s->coherent)));      // per-chain counters | per-wavefront shards (kernels.h: lean_scalars)
    HIPCKD(hipMemsetAsync(s->acc_count, 0, ((size_t)s->n_local + ACC_SHARDS) * sizeof(uint32_t), s->stream));
    HIPCKD(hipMemsetAsync(s->counters, 0, 8 * sizeof(unsigned long long), s->stream));
    if (want_om) {
        if (!s->om) CKD(s->mem.alloc(&s->om, (size_t)s->world * 2 * s->n_local));
        CKD(s->mem.alloc(&s->sel, 8));
        // (behind the state: one (value, index) pair per workgroup of a pass for the first maximum)
        const size_t sel_bytes = sizeof(SelState) + (size_t)sel_blocks(s->N) * (sizeof(double) + sizeof(uint32_t));
        CKD(s->mem.alloc(&s->sel_state, sel_bytes));
        HIPCKD(hipMemsetAsync(s->sel_state, 0, sel_bytes, s->stream));
        CKD(s->mem.alloc(&s->olist, (size_t)s->n_local + 1));
    }
    // update records drawn ahead (plan_kernel) for the fused device kernels, while a launch is latency bound.  Measured
    // on cfg2's target (one wavefront per chain): 11.4 vs 11.8 us/generation at N=2048, 15.9 vs 16.4 at 8192, 24.9 vs
    // 25.3 at 16384; from 32768 chains per GPU the records' extra 64 B per update cost more than the shorter critical
    // path gains (42.7 vs 41.6, 77.9 vs 75.8 at 65536).
    static const bool no_plan = test_path("noplan") || test_path("noperm");
    const uint32_t plan_max_local = test_path("planall") ? 0xFFFFFFFFu : 16384u;
    s->win_K = PERM_CHUNK;
    s->plan_on = !no_plan && s->shape.idx == 3 && s->n_local <= plan_max_local &&
                 (cfg->algo == BPM_ALGO_DREAM ? cfg->del_pairs <= 5 : cfg->algo == BPM_ALGO_DEMC) &&
                 // (a single-rank host-callback sampler too: the update kernel compiled around a likelihood given as HIP source reads them, bpm_set_device_likelihood)
                 (tid != BPM_TARGET_HOST_CALLBACK || s->world == 1);
    if (s->plan_on) {
        const size_t per_gen = (size_t)s->N * PLAN_WORDS * sizeof(uint32_t);
        s->win_K = (int)std::max<size_t>(1, std::min<size_t>((size_t)s->win_K, ((size_t)512 << 20) / per_gen));
        s->sorted_on = s->world > 1 && s->world <= (uint32_t)MAX_SEG && tid != BPM_TARGET_HOST_CALLBACK;
    }
    for (auto& B : s->tb) {
        CKD(s->mem.alloc(&B.perm, (size_t)s->win_K * s->N));
        CKD(s->mem.alloc(&B.inv, (size_t)s->win_K * s->N));
        if (s->plan_on) CKD(s->mem.alloc(&B.plan, (size_t)s->win_K * s->N * PLAN_WORDS));
        if (s->sorted_on) {
            CKD(s->mem.alloc(&B.sidx, (size_t)s->win_K * s->N));
            HIPCKD(hipMemsetAsync(B.sidx, 0xFF, (size_t)s->win_K * s->N * sizeof(uint32_t), s->stream));      // "no slot": plan_kernel skips such positions
            CKD(s->mem.alloc(&B.plan_count, (size_t)s->win_K * 2 * s->world));
            CKD(s->mem.alloc(&B.count_h, (size_t)s->win_K * 2 * s->world, MEM_PINNED));
        }
    }
    if (s->plan_on) s->plan_tab = s->tb[0].plan;       // (non-null from here on: "this sampler launches with records")
    CKD(s->mem.alloc(&s->gamma_tab, (size_t)s->dim + 1));
    if (cfg->algo == BPM_ALGO_DEMC_SYNC) CKD(s->mem.alloc(&s->x_next, row_d));
    {
        std::vector<double> gt(s->dim + 1, 0.0);      // dream.py:61, same operation order as the reference
        for (uint32_t dp = 1; dp <= s->dim; ++dp)
            gt[dp] = s->cfg.gamma_scale * 2.38 / std::sqrt(2. * (double)s->cfg.del_pairs * (double)dp);
        HIPCKD(hipMemcpyAsync(s->gamma_tab, gt.data(), gt.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIPCKD(hipStreamSynchronize(s->stream));
    }
    s->scratch_doubles = 4 * (size_t)s->ld + 64;
    CKD(s->mem.alloc(&s->scratch, s->scratch_doubles));
    if (tid == BPM_TARGET_HOST_CALLBACK) {
        CKD(s->mem.alloc(&s->prop_buf, row_d));
        CKD(s->mem.alloc(&s->aux_buf, 2 * (size_t)s->n_local));
        CKD(s->mem.alloc(&s->ids_buf, s->n_local));
        CKD(s->mem.alloc(&s->h_ids, s->n_local, MEM_PINNED));
        CKD(s->mem.alloc(&s->h_props, row_d, MEM_PINNED));
        CKD(s->mem.alloc(&s->h_ll, s->n_local, MEM_PINNED));
    }
    if (s->world > 1 && !cfg->nccl_uid) { bpm_destroy(s); return fail("bpm_create: nccl_uid required when world_size > 1"); }
    // Test mode: a uid starting with "BPMLOCAL" makes the ranks of a world handles of ONE process on one GPU;
    // bpm_local_group_step drives them in lock-step and does the all-gather with device copies.  It runs the
    // very kernels, layouts and host logic of a multi-GPU run (everything but RCCL) where only one GPU exists.
    if (cfg->nccl_uid && std::memcmp(cfg->nccl_uid, "BPMLOCAL", 8) == 0) {
#ifndef BPM_TEST_HOOKS
        bpm_destroy(s);
        return fail("bpm_create: local rank groups (a nccl_uid starting with BPMLOCAL, driven by bpm_local_group_step) exist only in the test variant of the library (include/bipymc_hip_test.h)");
#endif
        s->local_group = true;
        if (test_path("groupqueues") && s->dq) {
            bpm::DirectQueue* q = bpm::DirectQueue::create_private(cfg->device);
            if (q && q->kernel(reinterpret_cast<const void*>(perm_table_kernel)) && q->set_fence_kernel(reinterpret_cast<const void*>(queue_fence_kernel))) { s->dq = q; s->dq_private = true; }
            else if (q) bpm::DirectQueue::destroy_private(q);
        }
    } else if (cfg->nccl_uid && std::memcmp(cfg->nccl_uid, "BPMPUSH", 7) == 0) {
        // ranks in processes of their own WITHOUT an RCCL communicator: the push exchange is the only one (bpm_push_connect before the
        // first step).  What N processes sharing one GPU can use -- RCCL refuses two ranks on one device -- and what a caller without
        // RCCL on its nodes can use.
        if (!s->arena) { bpm_destroy(s); return fail("bpm_create: the push exchange needs a device target, 2..16 ranks and the pool-based samplers"); }
        s->push_no_rccl = true;
    } else
    if (cfg->nccl_uid) {      // world_size == 1 with a uid: a one-rank communicator (exercises the RCCL path on one GPU)
        CKD(load_rccl());
        ncclUniqueId id;
        std::memcpy(&id, cfg->nccl_uid, BPM_UID_BYTES);
        ncclResult_t r = g_rccl.CommInitRank(&s->comm, (int)s->world, id, (int)s->rank);
        if (r != ncclSuccess) { std::string m = std::string("ncclCommInitRank failed: ") + g_rccl.GetErrorString(r); bpm_destroy(s); return fail(m); }
    }
    // (a one-rank communicator takes the same path, so a one-GPU box can time and test it through RCCL)
    if ((s->world > 1 || s->comm) && cfg->algo != BPM_ALGO_DEMC_SYNC && cfg->target_id != BPM_TARGET_HOST_CALLBACK) {
        // BPM_EXCHANGE = dense | rows | replay (default replay): the initial value of bpm_set_exchange
        const char* xe = getenv("BPM_EXCHANGE");
        const bool want_dense = xe && std::strcmp(xe, "dense") == 0;
        const bool want_rows = xe && std::strcmp(xe, "rows") == 0;
        s->replay_enabled = !want_dense && !want_rows && s->shape.idx != SHAPE_WIDE;      // (wide rows: dense, or push once connected)
        s->sparse_enabled = !want_dense && want_rows && s->shape.idx != SHAPE_WIDE;
        CKD(s->mem.alloc(&s->accbits_all, (size_t)s->N));
        HIPCKD(hipMemsetAsync(s->accbits_all, 0, (size_t)s->N, s->stream));
        s->xnsub = 1u;
        // 4 sub-blocks: ~175 acceptances per counter and half generation at cfg2 cost the same on one GPU as 16
        // sub-blocks (23.2 vs 23.0 us/generation through a one-rank communicator; ONE counter: 34 us), and the
        // capacity margin, hence the bytes on the wire, shrinks with the count per sub-block (1.5 x instead of 2.2 x)
        const uint32_t nsub_max = 4u;
        while (2u * s->xnsub <= nsub_max && 2u * s->xnsub * 8u <= s->n_local) s->xnsub *= 2u;      // power of two, >= 8 chains each
        s->xcap_max = ((s->n_local + s->xnsub - 1u) / s->xnsub + 1u) & ~1u;    // every chain of a sub-block accepted
        s->xcap = s->xcap_max;                               // first chunk: cannot overflow; then sized from the counts seen
        const size_t pk_doubles = (size_t)s->world * s->xnsub * s->xstride();
        CKD(s->mem.alloc(&s->PK, pk_doubles));
        HIPCKD(hipMemsetAsync(s->PK, 0, pk_doubles * sizeof(double), s->stream));
        CKD(s->mem.alloc(&s->xstat, 2));
        HIPCKD(hipMemsetAsync(s->xstat, 0, 2 * sizeof(uint32_t), s->stream));
        CKD(s->mem.alloc(&s->ckpt_G, (size_t)s->world * s->L.blk));
        CKD(s->mem.alloc(&s->ckpt_ll, s->n_local));
        CKD(s->mem.alloc(&s->ckpt_acc, (size_t)s->n_local + ACC_SHARDS));
        CKD(s->mem.alloc(&s->ckpt_counters, 4));
    }
    HIPCKD(hipStreamSynchronize(s->stream));
    *out = s;
    return 0;
}

extern "C" int bpm_init_chains(bpm_handle_t s, const double* theta_0, const double* varepsilon) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!theta_0 || !varepsilon) return fail("bpm_init_chains: null argument");
    int jitter = 1;
    for (uint32_t j = 0; j < s->dim; ++j) {
        if (varepsilon[j] < 0.0) return fail("bpm_init_chains: varepsilon must be >= 0 (chain.py:22)");
        if (!(varepsilon[j] > 0.0)) jitter = 0;   // util.py:12: all > 0 or no noise at all
    }
    double* d_theta = s->scratch;
    double* d_var = s->scratch + s->ld;
    HIPCK(hipMemcpyAsync(d_theta, theta_0, s->dim * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(d_var, varepsilon, s->dim * sizeof(double), hipMemcpyHostToDevice, s->stream));
    const uint64_t n_elem = (uint64_t)s->n_local * s->ld;
    for (uint32_t r = 0; r < s->world; ++r) {   // every rank fills the whole replicated matrix: no exchange needed
        hipLaunchKernelGGL(init_jitter_kernel, dim3((unsigned)((n_elem + 255) / 256)), dim3(256), 0, s->stream, s->L,
                           r * s->n_local, (uint64_t)s->cfg.seed, d_theta, d_var, jitter);
    }
    HIPCK(hipGetLastError());
    CK(reset_history(s));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int bpm_set_state(bpm_handle_t s, const double* X) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!X) return fail("bpm_set_state: null argument");
    for (uint32_t r = 0; r < s->world; ++r) {
        HIPCK(hipMemcpy2DAsync(s->G + (uint64_t)r * s->L.blk, s->ld * sizeof(double),
                               X + (uint64_t)r * s->n_local * s->dim, s->dim * sizeof(double), s->dim * sizeof(double),
                               s->n_local, hipMemcpyHostToDevice, s->stream));
    }
    CK(reset_history(s));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int bpm_get_state(bpm_handle_t s, double* X) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!X) return fail("bpm_get_state: null argument");
    for (uint32_t r = 0; r < s->world; ++r) {
        HIPCK(hipMemcpy2DAsync(X + (uint64_t)r * s->n_local * s->dim, s->dim * sizeof(double),
                               s->G + (uint64_t)r * s->L.blk, s->ld * sizeof(double), s->dim * sizeof(double),
                               s->n_local, hipMemcpyDeviceToHost, s->stream));
    }
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int bpm_set_loglike(bpm_handle_t s, const double* ll_local) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!ll_local) return fail("bpm_set_loglike: null argument");
    // (the lean kernels never read the cache and refresh_ll would overwrite what a caller put there, a history row appended by position
    // would get its ln-likes by chain -- and nothing needs the call for a device target: the library evaluates the cache itself, reset_history)
    if (s->cfg.target_id != BPM_TARGET_HOST_CALLBACK)
        return fail("bpm_set_loglike: host-callback targets only (a sampler with a device target evaluates ln_like of its chains itself)");
    HIPCK(hipMemcpyAsync(s->ll, ll_local, s->n_local * sizeof(double), hipMemcpyHostToDevice, s->stream));
    // the log-like history row of the current state: row 0 after (re)initialisation, the LAST row after a warm start
    // (bpm_set_history with a host-callback target could only leave NaN there; older rows stay NaN: the reference's
    // checkpoint does not store log-likes, chain.py:59-70)
    if (last_row_is_state(s))
        HIPCK(hipMemcpyAsync(s->llhist + (size_t)(s->hist_rows - 1) * s->n_local, s->ll, s->n_local * sizeof(double),
                             hipMemcpyDeviceToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int bpm_get_loglike(bpm_handle_t s, double* ll_local) {
    CK(check_handle(s));
    CK(set_device(s));
    CK(refresh_ll(s));
    HIPCK(hipMemcpyAsync(ll_local, s->ll, s->n_local * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

static int ensure_perm_table(bpm_sampler* s, int64_t t, int64_t n_ahead);

extern "C" int bpm_begin_run(bpm_handle_t s, const bpm_run_opts_t* o) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->state_set) return fail("ERROR: chains not initilized");   // demc.py:65-66
    if (s->proposed) return fail("bpm_begin_run: a proposed half generation is awaiting bpm_commit");
    bpm_run_opts_t d;
    d.flip = 0.5; d.shuffle = 1; d._pad = 0; d.epsilon = -1.0; d.u_epsilon = -1.0; d.gamma = -1.0;
    if (o) d = *o;
    d.flip = std::min(1.0, std::max(0.0, d.flip));                                   // demc.py:73
    if (d.epsilon < 0.0) d.epsilon = (s->cfg.algo == BPM_ALGO_DREAM) ? 1e-12 : 1e-15;   // dream.py:40 / demc.py:161
    if (d.u_epsilon < 0.0) d.u_epsilon = 1e-2;                                        // dream.py:41
    if (!(d.gamma > 0.0)) d.gamma = 2.38 / std::sqrt(2.0 * (double)s->dim);            // demc.py:162
    s->opts = d;
    s->k_gen = 0;                                                                    // demc.py:78
    s->phase = 0;
    HIPCK(hipMemsetAsync(s->counters, 0, 4 * sizeof(unsigned long long), s->stream));
    HIPCK(hipMemsetAsync(s->acc_count, 0, ((size_t)s->n_local + ACC_SHARDS) * sizeof(uint32_t), s->stream));     // demc.py:67
    HIPCK(hipStreamSynchronize(s->stream));
    s->run_open = true;
    // the tables of the window this run starts in (and of the next one) are built from here on, beside whatever the caller does
    // before its first bpm_step
    if (s->cfg.algo != BPM_ALGO_DEMC_SYNC) CK(ensure_perm_table(s, s->t_abs, 1));
    return 0;
}

static int allgather_state(bpm_sampler* s) {
    if (!s->comm) return 0;
    NCCLCK(g_rccl.AllGather(s->G + (uint64_t)s->rank * s->L.blk, s->G, (size_t)s->L.blk, ncclDouble, s->comm, s->stream));
    return 0;
}

// Window W of the per-generation tables into buffer b, on the build stream.
static int build_window(bpm_sampler* s, int b, int64_t W, int shuffle) {
    bpm_sampler::TabBuf& B = s->tb[b];
    const int K = s->win_K;
    const int64_t t0 = W * K;
    hipStream_t bs = s->stream;
    PermKeys keys;
    for (int g = 0; g < K; ++g) keys.k[g] = make_perm_key(s->cfg.seed, (uint64_t)(t0 + g), s->N, shuffle != 0);
    for (int g = K; g < PERM_CHUNK; ++g) keys.k[g] = keys.k[0];
    const uint64_t n = (uint64_t)K * s->N;
    // the inverse tables (chain id -> position) serve launches with one work item per LOCAL chain: the ranks of a world (and the test path that takes
    // their kernel path on one GPU); a single-GPU sampler's buffer stays allocated (PhaseArgs::inv_tab is never null with tables) but is not filled
    static const bool force_mode1 = test_path("mode1");
    uint32_t* const inv_out = (s->world > 1 || force_mode1) ? B.inv : nullptr;
    if (g_disp.dq && !B.sidx) {
        // direct mode, records by position: the same two kernels as packets on the library's queue, in order with
        // the update kernels around them
        CK(launch_side(bs, perm_table_kernel, "perm_table_kernel", dim3((uint32_t)((n + 255) / 256)), 256, bpm::DirectQueue::FENCED, Then::KEEP, keys, K, s->N, B.perm, inv_out));
        if (B.plan) {
            const PlanParams pp{s->cfg.seed, (uint64_t)t0, (uint32_t)K, s->N, s->cfg.algo == BPM_ALGO_DREAM ? (uint32_t)s->cfg.del_pairs : 1u,
                                (s->cfg.algo == BPM_ALGO_DEMC && s->cfg.p_snooker > 0.0) ? 1u : 0u, 0u, 0u};
            CK(launch_side(bs, plan_kernel, "plan_kernel", dim3((uint32_t)((n + 255) / 256)), 256, bpm::DirectQueue::FENCED, Then::KEEP, pp, B.perm, B.plan, B.sidx));
        }
        B.W = W;
        B.shuffle = shuffle;
        g_disp.mark_acquire(true);      // (the update kernels read the tables)
        return 0;
    }
    // A rank of a world with owner-sorted records (B.sidx) builds on the HIP stream even while its generation loop runs on the library's
    // own queue (push exchange): the slot table comes from plan_slot_kernel and the launch sizes of the window must reach the HOST
    // (pinned copy + event), neither of which the queue path above does -- it once took a window with an unbuilt slot table (records
    // scattered to garbage slots: a memory fault after 64 generations, the first window built inside direct mode).  Queue drained
    // before, stream drained after: once per 64 generations.
    StreamSection sec(s);
    CK(sec.rc);
    hipLaunchKernelGGL(perm_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, bs, keys, (uint32_t)K, s->N, B.perm, inv_out);
    HIPCK(hipGetLastError());
    if (B.plan) {
        // (push exchange: nobody replays another rank's updates -- only this rank's own run of the owner-sorted records is built;
        // a window remembers it, and a change of the exchange mode rebuilds)
        const bool own_only = B.sidx != nullptr && s->push_enabled && s->push_connected;
        B.own_only = own_only;
        if (B.sidx) {              // world > 1: every position's slot in the owner-sorted order, every rank's counts (they size the launches)
            if (own_only) {        // this rank's positions only: the other ranks' counts stay zero, its own run starts at the half's offset
                const uint32_t n_chunks = ((s->N + 1u) / 2u + SLOT_CHUNK - 1u) / SLOT_CHUNK;
                if (!B.chunk_count) CK(regrow(s, &B.chunk_count, (size_t)s->win_K * 2 * n_chunks, 0, false));
                HIPCK(hipMemsetAsync(B.plan_count, 0, (size_t)K * 2 * s->world * sizeof(uint32_t), bs));
                for (uint32_t assign = 0; assign < 2; ++assign)
                    hipLaunchKernelGGL(plan_slot_own_kernel, dim3(n_chunks, 2, (unsigned)K), dim3(SLOT_CHUNK), 0, bs, B.perm, s->N, s->lo, s->n_local, s->world,
                                       s->rank, n_chunks, B.chunk_count, B.sidx, B.plan_count, assign);
            } else {
                hipLaunchKernelGGL(plan_slot_kernel, dim3(2, (unsigned)K), dim3(PLAN_LOCAL_THREADS), 0, bs, B.perm, s->N, s->n_local, s->world,
                                   B.sidx, B.plan_count);
            }
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(B.count_h, B.plan_count, (size_t)K * 2 * s->world * sizeof(uint32_t), hipMemcpyDeviceToHost, bs));
        }
        PlanParams pp{s->cfg.seed, (uint64_t)t0, (uint32_t)K, s->N, s->cfg.algo == BPM_ALGO_DREAM ? (uint32_t)s->cfg.del_pairs : 1u,
                      (s->cfg.algo == BPM_ALGO_DEMC && s->cfg.p_snooker > 0.0) ? 1u : 0u, own_only ? s->lo : 0u, own_only ? s->n_local : 0u};
        hipLaunchKernelGGL(plan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, bs, pp, B.perm, B.plan, B.sidx);
        HIPCK(hipGetLastError());
    }
    HIPCK(hipEventRecord(B.built, bs));
    CK(sec.end());
    B.W = W;
    B.shuffle = shuffle;
    return 0;
}

// The tables of generation t are current on the update stream; on entering a window the next one is started on the build
// stream.  In a run that crosses windows the update kernels therefore find every window but the very first already built
// (bpm_begin_run starts that one), and a rank of a world finds its launch sizes on the host without stalling.
static int ensure_perm_table(bpm_sampler* s, int64_t t, int64_t /*n_ahead*/) {
    const int shuffle = s->opts.shuffle != 0 ? 1 : 0;
    if (s->cur >= 0 && s->tab_shuffle == shuffle && t >= s->tab_t0 && t < s->tab_t0 + s->tab_K) return 0;
    const int K = s->win_K;
    const int64_t W = t / K;
    const int b = (int)(W & 1);
    bpm_sampler::TabBuf& B = s->tb[b];
    const bool want_own = B.sidx != nullptr && s->push_enabled && s->push_connected;
    if (B.W != W || B.shuffle != shuffle || (B.sidx && B.own_only && !want_own)) CK(build_window(s, b, W, shuffle));
    if (B.sidx) HIPCK(hipEventSynchronize(B.built));              // the window's launch sizes (count_h)
    s->cur = b;
    s->perm_tab = B.perm; s->inv_tab = B.inv; s->plan_tab = B.plan; s->plan_count_h = B.count_h;
    s->tab_t0 = W * K;
    s->tab_K = K;
    s->tab_shuffle = shuffle;
    bpm_sampler::TabBuf& Bn = s->tb[b ^ 1];
    if (Bn.W != W + 1 || Bn.shuffle != shuffle || (Bn.sidx && Bn.own_only && !want_own)) CK(build_window(s, b ^ 1, W + 1, shuffle));
    return 0;
}

// Everything of one generation that is decided on the host: flip, shuffle key, group ranges
// (demc.py:81-86,95-100), gating flags (dream.py:92,123), history row.
// totals (cr_state) + `cnt` partial sums of one generation -> cr_state: cr_final_kernel on the queue the generation loop runs on
static int launch_cr_final(bpm_sampler* s, const double* src, uint32_t cnt) {
    const uint32_t n_cr = (uint32_t)s->cfg.n_cr;
    const int fence = s->dq_fence | bpm::DirectQueue::ACQUIRE;
    // (ROUNDS = partials per lane, the next power of two: a partial beyond cnt reads as +0.0, the sums do not depend on the choice)
    typedef void (*FinalK)(const double*, const double*, uint32_t, uint32_t, double*);
    const uint32_t rounds = (cnt + WAVE - 1) / WAVE;
    const FinalK kfn = rounds <= 1 ? cr_final_kernel<1> : (rounds <= 2 ? cr_final_kernel<2> : (rounds <= 4 ? cr_final_kernel<4> : cr_final_kernel<8>));
    return launch_side(s->stream, kfn, "cr_final_kernel", dim3(1), WAVE, fence, Then::NO_ACQUIRE, s->cr_state, src, cnt, n_cr, s->cr_state);
}
// the fold nobody consumed (bpm_sampler::cr_pending)
static int cr_flush_pending(bpm_sampler* s) {
    if (!s->cr_pending) return 0;
    s->cr_pending = false;
    return launch_cr_final(s, s->cr_pend_src, s->cr_pend_cnt);
}

static int prepare_generation(bpm_sampler* s, int64_t n_ahead) {
    const bool dream = s->cfg.algo == BPM_ALGO_DREAM;
    const uint64_t t = (uint64_t)s->t_abs;
    const bool sync = s->cfg.algo == BPM_ALGO_DEMC_SYNC;
    if (!sync) CK(ensure_perm_table(s, s->t_abs, n_ahead));
    const bool flip = flip_draw(s->cfg.seed, t, s->opts.flip);
    const PermKey pk = make_perm_key(s->cfg.seed, t, s->N, s->opts.shuffle != 0);
    const uint32_t n_first = (s->N + 1) / 2, n_second = s->N - n_first;    // np.array_split: first gets ceil
    uint32_t a_off = 0, a_n = n_first, b_off = n_first, b_n = n_second;
    if (flip) { std::swap(a_off, b_off); std::swap(a_n, b_n); }
    const bool adapt_on = dream && (s->cfg.burnin_gen > s->k_gen);          // dream.py:92
    s->gen_adapt_on = adapt_on;
    // the CR statistics of a generation are reduced only when some update could contribute: while the chains' histories are not longer than
    // n_cr_gen (dream.py:123) every slot says "no update" and the reduction would leave p_cr, delta_m and n_cr_updates as they are -- two
    // dependent dispatches (6 us at cfg2) for nothing, in the first n_cr_gen generations of every fresh run
    s->gen_cr_reduce = adapt_on && s->rows_logical > s->cfg.n_cr_gen;
    if (adapt_on && s->w_rows != s->rows_logical) {
        if (!history_resident(s))
            return fail("CR adaptation needs the chain history (keep_history=1) to rebuild its moments");
        // A thinned history holds every hist_stride-th row: the moments of the stored rows, with m2 scaled by logical / stored rows, so that
        // m2 / rows_logical -- what the in-kernel update, which counts with hist_len = rows_logical, goes on from -- is the variance of the
        // stored rows ("Deviations").  A row per generation: x 1.0, the same bits as ever.
        const double m2_scale = s->hist_rows == s->rows_logical ? 1.0 : (double)s->rows_logical / (double)s->hist_rows;
        const uint64_t n_elem = (uint64_t)s->n_local * s->ld;
        StreamSection sec(s);
        CK(sec.rc);
        CK(normalize_history(s, 0, s->hist_rows));
        hipLaunchKernelGGL(welford_rebuild_kernel, dim3((unsigned)((n_elem + 255) / 256)), dim3(256), 0, s->stream,
                           s->hist, n_elem, n_elem, (uint32_t)s->hist_rows, s->ld, m2_scale, s->w_mean, s->w_m2);
        HIPCK(hipGetLastError());
        CK(sec.end());
        s->w_rows = s->rows_logical;
    }
    CK(ensure_gen_sums(s, s->rows_logical + 1));
    double* hist_row = nullptr;
    double* llhist_row = nullptr;
    if (generation_appends(s)) {      // (a thinned history skips the generations between its rows: null pointers, the kernels append nothing)
        CK(ensure_history(s, s->hist_rows + 1));
        hist_row = s->hist + (uint64_t)s->hist_rows * s->n_local * s->ld;
        llhist_row = s->llhist + (uint64_t)s->hist_rows * s->n_local;
        s->hist_tag[(size_t)s->hist_rows] = -1;      // (how the row about to be appended has to be read: decided in finish_generation)
    }
    for (int ph = 0; ph < 2; ++ph) {
        PhaseArgs& a = s->cur_args[ph];
        std::memset(&a, 0, sizeof(a));
        a.set_L(s->L);
        a.ll = s->ll;
        a.hist_row = hist_row;
        a.llhist_row = llhist_row;
        a.w_mean = s->w_mean;
        a.w_m2 = s->w_m2;
        a.tparams = s->tparams;
        a.cr_state = s->cr_state;
        a.counters = s->counters;
        a.acc_count = s->acc_count;
        a.prop_buf = s->prop_buf;
        a.aux_buf = s->aux_buf;
        a.ids_buf = s->ids_buf;
        trace_set(a, s->trace_i32, s->trace_f64, s->trace_mask);      // (test variant only: the product's argument block has no trace fields)
        a.pk = pk;
        a.perm_tab = s->perm_tab + (uint64_t)(s->t_abs - s->tab_t0) * s->N;
        a.inv_tab = s->inv_tab + (uint64_t)(s->t_abs - s->tab_t0) * s->N;
        a.plan = (s->plan_tab && !s->sorted_on) ? s->plan_tab + (uint64_t)(s->t_abs - s->tab_t0) * s->N * PLAN_WORDS : nullptr;   // records BY POSITION
        a.rec_tab = a.plan;
        { static const bool no_tab = test_path("noperm");
          if (no_tab) { a.perm_tab = nullptr; a.inv_tab = nullptr; } }
        a.gamma_tab = s->gamma_tab;
        a.stamps = s->stamps;
        for (int m = 0; m < s->cfg.n_cr && m < MAX_CR; ++m)
            a.thr[m] = (uint32_t)std::floor(((double)(m + 1) / (double)s->cfg.n_cr) * 65536.0);   // dream.py:113
        a.seed = s->cfg.seed;
        a.t = t;
        a.k = (uint32_t)s->k_gen;
        a.N = s->N;
        a.lo = s->lo;
        a.upd_off = ph == 0 ? a_off : b_off;
        a.n_upd = ph == 0 ? a_n : b_n;
        a.pool_off = ph == 0 ? b_off : a_off;
        a.M = ph == 0 ? b_n : a_n;
        // mode 1 (work item = local chain, filtered by its position) is what world_size > 1 uses;
        // BPM_TEST_PATHS=mode1 selects it on one GPU so the sharded kernel path can be tested there
        static const bool force_mode1 = test_path("mode1");
        const bool by_chain = s->world > 1 || force_mode1;
        a.mode = by_chain ? 1u : 0u;
        a.n_items = by_chain ? s->n_local : a.n_upd;
        a.rec_off = a.upd_off;
        if (s->sorted_on && s->plan_tab) {
            // a rank of a world with owner-sorted records: its updates of this half generation are one contiguous run of records --
            // item k -> its k-th update: the single-GPU launch shape (no idle items, no position lookup); the other ranks' runs are
            // what the replay kernel walks
            const uint32_t grp = a.upd_off == 0 ? 0u : 1u;
            const uint32_t* cnt = s->plan_count_h + ((uint64_t)(s->t_abs - s->tab_t0) * 2 + grp) * s->world;   // (pinned copy, complete:
                                                                                                          // ensure_perm_table waited for the build)
            uint32_t acc = a.upd_off;
            for (uint32_t r = 0; r < s->world; ++r) { a.seg_off[r] = acc; acc += cnt[r]; }
            for (uint32_t r = s->world; r <= (uint32_t)MAX_SEG; ++r) a.seg_off[r] = acc;
            // (the counts size this rank's launch: a window whose slot pass did not run -- round 3's first push runs, DESIGN.md section 6 -- must be
            // an error here, not a launch of garbage size)
            if (acc > a.upd_off + a.n_upd || cnt[s->rank] > a.n_upd)
                return fail("owner-sorted update records: the counts of generation " + std::to_string((long long)s->t_abs) + " exceed its half generation (window not built?)");
            a.n_seg = s->world; a.seg_me = s->rank; a.acc_by_item = 1u;
            a.rec_sorted = s->plan_tab + (uint64_t)(s->t_abs - s->tab_t0) * s->N * PLAN_WORDS;
            a.rec_tab = a.rec_sorted + (uint64_t)a.seg_off[s->rank] * PLAN_WORDS;
            a.rec_off = 0u;
            a.n_items = cnt[s->rank];
            a.mode = 0u;
        }
        // (while the outlier check is due every few generations -- DREAM burn-in with outlier_every > 0 -- the ln-like goes by chain: the check sums
        // every chain's ln-like history, and reads the state rows of the few chains it resets where they lie: outlier_row_keys)
        const bool outlier_phase = dream && s->cfg.outlier_every > 0 && s->k_gen < s->cfg.burnin_gen;
        a.hist_by_pos = (s->hist_by_pos && (s->cfg.target_id != BPM_TARGET_HOST_CALLBACK || g_disp.user_cur == s) && hist_row != nullptr && !by_chain && !sync &&
                         s->trace_i32 == nullptr) ? (outlier_phase ? 2u : 1u) : 0u;
        { static const bool wt8 = test_path("wt8"); a.wt = g_disp.wt_stores ? (wt8 ? 1u : 2u) : 0u; }
        a.lean = s->lean ? 1u : 0u;
        a.algo = (uint32_t)s->cfg.algo;
        a.P = (uint32_t)s->cfg.del_pairs;
        a.n_cr = (uint32_t)s->cfg.n_cr;
        a.adapt_on = adapt_on ? 1u : 0u;
        a.cr_gate = (s->rows_logical > s->cfg.n_cr_gen) ? 1u : 0u;          // dream.py:123
        a.hist_len = (uint32_t)s->rows_logical;
        a.gamma_scale = s->cfg.gamma_scale;
        a.gamma_demc = s->opts.gamma;
        a.epsilon = s->opts.epsilon;
        a.u_epsilon = s->opts.u_epsilon;
        a.p_snooker = s->cfg.p_snooker;
        if (s->replay_active) a.accbits = s->accbits_all + (uint64_t)s->rank * s->n_local;
        if (s->push_active) { a.peer_tab = s->tab_peerG; a.n_peers = s->world - 1u; }
        if (s->sparse_active) {
            a.pack = s->PK + (uint64_t)s->rank * s->xnsub * s->xstride();
            a.pack_cap = s->xcap;
            a.pack_nsub = s->xnsub;
            a.pack_stride = s->xstride();
        }
        a.cr_part1 = nullptr; a.cr_chunk0 = 0u; a.cr_n1 = s->cr_n1;
        a.cr_fold_part = nullptr; a.cr_fold_tot = nullptr; a.cr_fold_out = nullptr; a.cr_fold_nb = 0u;
        if (sync) {      // samplers.py:261-308: one launch, every local chain against all other chains, updates banked
            a.algo = (uint32_t)BPM_ALGO_DEMC;
            a.mode = 2u;
            a.n_items = ph == 0 ? s->n_local : 0u;
            a.perm_tab = nullptr; a.inv_tab = nullptr; a.pk.on = 0u;
            a.upd_off = 0; a.n_upd = s->N; a.pool_off = 0; a.M = s->N - 1;
            a.x_next = s->x_next;
        }
    }
    // The flavour of each update launch, chosen HERE and nowhere else (kernels.h: choose_flavour): launch_update launches what cur_hot says, and the plan
    // of the CR reduction below is a function of it.  The looped wide-row kernel and the synchronous mode have the general flavour only, and so has a
    // host-callback sampler nothing launches an update kernel for (cur_launch == nullptr: its generation is the proposal and commit kernels).
    static const bool no_hot = test_path("nohot"), cr_slots = test_path("crslots");
    const bool user_driven = g_disp.user_cur == s;      // the update kernel compiled around a HIP-source likelihood drives this (host-callback) sampler
    const UserLikelihood::Fused& mod = s->like.fused;
    s->cur_launch = user_driven ? launch_user_fused : pick_fused(s);
    for (int ph = 0; ph < 2; ++ph) {
        const PhaseArgs& a = s->cur_args[ph];
        int f = (no_hot || sync || s->shape.idx == SHAPE_WIDE || !s->cur_launch) ? FLAVOUR_GENERAL : choose_flavour(a, dream, s->shape.lpc == WAVE && s->shape.dpl == 2);
        // a run-time module holds the general instantiation, ONE steady-state flavour and (DREAM) ONE burn-in flavour, each compiled with update
        // records exactly when this sampler builds them (plan_on)
        if (user_driven && !(((flavour_is_steady(f) && mod.hot != nullptr) || (hot_is_adapt(f) && mod.adapt != nullptr)) && (a.rec_tab != nullptr) == s->plan_on))
            f = FLAVOUR_GENERAL;
        s->cur_hot[ph] = f;
    }
    // CR reduction, level 1 (kernels.h): written by the update kernels themselves when EVERY non-empty launch of the generation has a burn-in flavour
    // (HOT 3 / 4) of a shape that sums (crp_shape), else computed from the slots in finish_generation
    if (s->cr_p1) s->cr_p1_cur = s->cr_p1 + (size_t)(s->t_abs & 1) * 2 * MAX_CR * s->cr_n1;
    s->gen_cr_inkernel = s->gen_cr_reduce && !cr_slots && crp_shape(s->shape.lpc, s->shape.dpl);
    for (int ph = 0; ph < 2; ++ph)
        if (s->cur_args[ph].n_items > 0 && !hot_is_adapt(s->cur_hot[ph])) s->gen_cr_inkernel = false;
    if (s->gen_cr_inkernel) {
        const uint32_t n_first = (s->N + 1u) / 2u;
        for (int ph = 0; ph < 2; ++ph) {
            PhaseArgs& a = s->cur_args[ph];
            a.cr_part1 = s->cr_p1_cur;
            a.cr_chunk0 = a.upd_off == 0u ? 0u : cr_chunks_of(n_first, s->cr_g1);
        }
    }
    // Two rules that differ on purpose.  A SHIPPED target's launch keeps its burn-in flavour in every adapting generation, whether or not level 1 is
    // written in-kernel (cr_part1 may be null: the kernel then writes the chains' slots).  A run-time MODULE's burn-in flavour is taken only when
    // in-kernel level 1 was planned: its other adapting generations run on the general instantiation.
    if (user_driven && !s->gen_cr_inkernel)
        for (int ph = 0; ph < 2; ++ph)
            if (hot_is_adapt(s->cur_hot[ph])) s->cur_hot[ph] = FLAVOUR_GENERAL;
    // a pending fold of the previous generation's CR statistics (bpm_sampler::cr_pending): consumed by this generation's first update launch when that one
    // has a flavour that can (a burn-in flavour that sums level 1 itself: HOT 3 / 4), else dispatched now, ahead of the update launches
    if (s->cr_pending) {
        PhaseArgs& a0 = s->cur_args[0];
        if (s->gen_cr_inkernel && a0.n_items > 0 && a0.cr_part1 != nullptr) {
            a0.cr_fold_part = s->cr_pend_src; a0.cr_fold_nb = s->cr_pend_cnt; a0.cr_fold_tot = s->cr_state; a0.cr_fold_out = s->cr_state_alt;
            std::swap(s->cr_state, s->cr_state_alt);
            s->cur_args[1].cr_state = s->cr_state;      // (the second launch reads what workgroup 0 of the first one stored; the first takes p_cr from its own fold)
            s->cr_pending = false;
        } else {
            CK(cr_flush_pending(s));
        }
    }
    return 0;
}

static int finish_generation(bpm_sampler* s) {
    if (s->lean) s->ll_stale = true;
    if (s->gen_adapt_on && !s->gen_cr_reduce) s->w_rows += 1;       // (the update kernels advanced the Welford moments all the same)
    if (s->gen_cr_reduce) {
        // this generation's CR statistics -> totals, p_cr (kernels.h: "CR reduction"): level 1 came out of the update kernels themselves
        // (gen_cr_inkernel) or is computed from the slots here, cr_mid_kernel passes bring more than 1024 partial sums down, cr_final_kernel folds
        const uint32_t n_cr = (uint32_t)s->cfg.n_cr;
        const int fence = s->dq_fence | bpm::DirectQueue::ACQUIRE;      // (a few hundred bytes, all through agent-scope stores: no release on these packets)
        Dispatch& d = g_disp;
        if (d.dq) d.mark_acquire(false);
        // (every flavour that does not write level 1 itself writes the chains' slots: kernels.h, finish_update<..., CRP_W>)
        const bool level1_from_slots = !s->gen_cr_inkernel;
        if (level1_from_slots) {
            const PhaseArgs& a0 = s->cur_args[0];
            typedef void (*L1K)(Layout, PermKey, const uint32_t*, uint32_t, uint32_t, uint32_t, double*);
            const L1K l1 = s->cr_g1 == 4u ? cr_level1_kernel<4> : (s->cr_g1 == 16u ? cr_level1_kernel<16> : cr_level1_kernel<64>);
            CK(launch_side(s->stream, l1, "cr_level1_kernel", dim3((uint32_t)(((uint64_t)s->cr_n1 * s->cr_g1 + CR_L1_THREADS - 1) / CR_L1_THREADS)), CR_L1_THREADS, fence, Then::KEEP,
                           s->L, a0.pk, a0.perm_tab, s->N, n_cr, s->cr_n1, s->cr_p1_cur));
        }
        const double* src = s->cr_p1_cur;
        uint32_t cnt = s->cr_n1;
        int flip = 0;
        while (cnt > CR_FINAL_MAX) {
            const uint32_t nn = (cnt + WAVE - 1) / WAVE;
            double* dst = s->cr_p2[flip];
            CK(launch_side(s->stream, cr_mid_kernel, "cr_mid_kernel", dim3(nn), WAVE, fence, Then::KEEP, src, cnt, n_cr, nn, dst));
            src = dst; cnt = nn; flip ^= 1;
        }
        static const bool no_defer = test_path("crnofold");
        if (!level1_from_slots && cnt <= CR_FINAL_MAX && !d.call_last_gen && !no_defer) {
            // consumer-side fold: no dispatch -- the next generation's first update launch folds (prepare_generation), or cr_flush_pending
            s->cr_pending = true;
            s->cr_pend_src = src;
            s->cr_pend_cnt = cnt;
        } else {
            CK(launch_cr_final(s, src, cnt));
        }
        s->w_rows += 1;
    }
    if (s->cfg.running_moments) CK(push_gen_sums(s, s->rows_logical));      // (the row this generation appended: index rows_logical)
    if (generation_appends(s)) {
        if (s->cur_args[0].hist_by_pos || s->cur_args[1].hist_by_pos)      // appended by position: generation t_abs, ln-like by chain?, shuffle switch
            s->hist_tag[(size_t)s->hist_rows] = (s->t_abs << 2) | ((s->cur_args[0].hist_by_pos | s->cur_args[1].hist_by_pos) == 2u ? 2 : 0) |
                                                (s->opts.shuffle != 0 ? 1 : 0);
        s->hist_rows += 1;
    }
    s->rows_logical += 1;
    s->k_gen += 1;      // demc.py:134
    s->t_abs += 1;
    s->outlier_due = s->cfg.algo == BPM_ALGO_DREAM && s->cfg.outlier_every > 0 && s->k_gen < s->cfg.burnin_gen &&
                     s->k_gen % s->cfg.outlier_every == 0;
    return 0;
}

// ---- generation drivers ---------------------------------------------------------------------------------
// A Group is what advances in lock-step: the single handle of a process (exchange = RCCL on its stream) or, in
// the local-group test mode, the R handles that stand for the R ranks (exchange = device copies).  Both run the
// SAME code below, so what the one-GPU tests verify is what a multi-GPU run executes, transport aside.
struct Group {
    bpm_sampler** h;
    int R;
    bool rccl;
};
constexpr int64_t SPARSE_CHUNK = 64;

// BPM_TEST_PATHS=serial (tools/emulate_ranks.py): the emulated ranks of a local group take turns on the GPU, so that a kernel
// trace shows each rank's kernels as they would run on a GPU of their own
static bool local_serial(const Group& g) {
    static const bool on = test_path("serial");
    return on && g.R > 1;
}

static int group_sync(const Group& g) {
    for (int r = 0; r < g.R; ++r) HIPCK(hipStreamSynchronize(g.h[r]->stream));
    return 0;
}

// ---- push exchange ---------------------------------------------------------------------------------------------------------
// bound of every cross-rank wait inside push_sync_kernel, in ticks of the 100 MHz constant clock (BPM_PUSH_TIMEOUT_S, default 30 s:
// ranks of a world start their step calls within seconds of each other -- the host-side classes put a communicator barrier in front)
static unsigned long long push_timeout_ticks() {
    static const double v = getenv("BPM_PUSH_TIMEOUT_S") ? atof(getenv("BPM_PUSH_TIMEOUT_S")) : 30.0;
    return (unsigned long long)(std::max(0.001, v) * 1e8);
}
// one push_sync_kernel of rank s: on the library's own queue when the generation loop runs there, else on the sampler's stream
static int launch_push_sync(bpm_sampler* s, unsigned long long seq, bool notify, bool wait) {
    const unsigned long long* ctab = s->tab_all + MAX_SEG;
    // NO fences on the queue's packet (the barrier bit orders it behind the update kernel, whose own packet released): the kernel reads and
    // writes nothing but the flags, with system-scope atomics that pass the caches; the update kernel that follows acquires.
    // (With acquire + release at system scope here as well a hand-over measured 10.0 us instead of 3.8 with agent-scope fences:
    // profiles/r03_push_barrier_cost.txt.)
    return launch_side(s->stream, push_sync_kernel, "push_sync_kernel", dim3(1), WAVE, 0, Then::ACQUIRE,
                       s->ctrl, ctab, s->world, s->rank, seq, notify ? 1u : 0u, wait ? 1u : 0u, push_timeout_ticks());
}
// The cross-rank barrier of the push exchange: "every rank has finished -- and pushed -- everything it enqueued before this point".
// A process per rank: one kernel announces and waits.  A local group (R handles of one process on one GPU, possibly sharing hardware
// queues): all ranks announce, the host joins the streams, all ranks wait -- the waits then find their flags set, no kernel ever
// spins on a kernel queued behind it.
static inline void bind_rank_queue(bpm_sampler* s) { if (g_disp.group_direct) g_disp.dq = s->dq; }
static int push_barrier(const Group& g) {
    for (int r = 0; r < g.R; ++r) g.h[r]->push_seq += 1;
    if (g.R == 1) return launch_push_sync(g.h[0], g.h[0]->push_seq, true, true);
    if (g_disp.group_direct) {          // every rank on a queue of its own: the kernels wait for each other across the queues
        for (int r = 0; r < g.R; ++r) { bind_rank_queue(g.h[r]); CK(launch_push_sync(g.h[r], g.h[r]->push_seq, true, true)); g.h[r]->dq->flush(); }
        return 0;
    }
    for (int r = 0; r < g.R; ++r) CK(launch_push_sync(g.h[r], g.h[r]->push_seq, true, false));
    CK(group_sync(g));
    for (int r = 0; r < g.R; ++r) CK(launch_push_sync(g.h[r], g.h[r]->push_seq, false, true));
    return 0;
}
// has a wait of this rank's sync kernels run into its limit? (read with the queue / stream drained)
static int push_check_error(bpm_sampler* s) {
    if (!s->push_connected) return 0;
    unsigned long long e = 0;
    HIPCK(hipMemcpy(&e, &s->ctrl->err, sizeof(e), hipMemcpyDeviceToHost));
    if (e != 0) s->push_failed = true;
    if (e >= PUSH_ERR_CLOSED)
        return fail("push exchange: rank " + std::to_string((long long)(e - PUSH_ERR_CLOSED)) + " closed its sampler (bpm_destroy) while rank " + std::to_string(s->rank) +
                    " was still exchanging with it: the ranks of a world must make the same sequence of calls; the replicas are no longer consistent");
    if (e != 0) return fail("push exchange: rank " + std::to_string(s->rank) + " waited longer than the limit for rank " + std::to_string((long long)e - 1) +
                            " (a rank that died, or ranks that entered bpm_step more than BPM_PUSH_TIMEOUT_S apart); the replicas are no longer consistent");
    return 0;
}

// The shuffle keys of the history rows for the outlier check's kernels (identity for what lies in chain order): state rows and ln-like rows have
// a key each (hist_tag).  On the sampler's stream, from a host vector that outlives the copy.
static int outlier_row_keys(bpm_sampler* s) {
    s->okeys_x = s->okeys_ll = false;
    if (!s->hist_by_pos) return 0;
    const size_t rows = (size_t)s->hist_rows;
    HIPCK(hipStreamSynchronize(s->stream));      // (the previous check's kernels and copy are done with okeys / okeys_host)
    if (rows > s->okeys_cap) {
        const size_t cap = std::max<size_t>(rows + rows / 2, 256);
        CK(regrow(s, &s->okeys, 2 * cap, 0, false));
        s->okeys_cap = cap;
    }
    PermKey id{};
    id.n = s->N; id.nbits = perm_nbits(s->N); id.on = 0u;
    s->okeys_host.assign(2 * s->okeys_cap, id);
    for (size_t r = 0; r < rows; ++r) {
        const int64_t tag = r < s->hist_tag.size() ? s->hist_tag[r] : -1;
        if (tag < 0) continue;
        const PermKey k = make_perm_key(s->cfg.seed, (uint64_t)(tag >> 2), s->N, (tag & 1) != 0);
        s->okeys_host[r] = k;
        s->okeys_x = true;
        if ((tag & 2) == 0) { s->okeys_host[s->okeys_cap + r] = k; s->okeys_ll = true; }
    }
    if (s->okeys_x) HIPCK(hipMemcpyAsync(s->okeys, s->okeys_host.data(), 2 * s->okeys_cap * sizeof(PermKey), hipMemcpyHostToDevice, s->stream));
    return 0;
}
// the eight passes of the radix select (+ first maximum) over s->om -> s->sel
static void launch_outlier_select(bpm_sampler* s, const SelRanks& R) {
    const uint32_t nblk = sel_blocks(s->N);
    for (int pass = 0; pass < 8; ++pass)
        hipLaunchKernelGGL(outlier_select_pass_kernel, dim3(nblk), dim3(SEL_THREADS), 0, s->stream, s->om, s->n_local, s->N, pass, R,
                           reinterpret_cast<SelState*>(s->sel_state), s->sel);
}

// DREAM outlier-chain reset (Vrugt et al. 2009; extension): chains whose mean ln_like over the last half of their history
// lies below Q1 - 2 IQR (quartiles over all N chains, np.percentile's interpolation) restart from the best chain's state.
// Everything stays on the device and on the samplers' streams: omega of the local chains, all-gather of the (omega | ln_like)
// blocks (RCCL, or device copies in a local group), radix select of the four order statistics + first argmax, reset.
static int group_outlier_check(const Group& g) {
    bpm_sampler* s0 = g.h[0];
    const uint32_t N = s0->N;
    for (int r = 0; r < g.R; ++r) {
        bpm_sampler* s = g.h[r];
        s->outlier_due = false;
        if (!s->cfg.keep_history || s->hist_rows != s->rows_logical) return fail("outlier detection needs the chain history");
        CK(outlier_row_keys(s));                             // (rows appended by position are read where they lie)
        CK(refresh_ll(s));                                   // (the (omega | ln-like) block carries the chains' current ln-like)
        const uint32_t rows = (uint32_t)s->hist_rows, r0 = rows / 2;
        hipLaunchKernelGGL(outlier_omega_kernel, dim3((s->n_local + 255) / 256), dim3(256), 0, s->stream, s->llhist, s->ll, s->n_local, r0, rows,
                           s->okeys_ll ? (const PermKey*)(s->okeys + s->okeys_cap) : (const PermKey*)nullptr, s->om + (size_t)s->rank * 2 * s->n_local);
        HIPCK(hipGetLastError());
    }
    if (s0->push_active) {
        // push exchange: every rank writes its (omega | ln-like) block into the others' om buffers, then the cross-rank barrier
        for (int r = 0; r < g.R; ++r) {
            bpm_sampler* s = g.h[r];
            const uint32_t n = 2u * s->n_local;
            hipLaunchKernelGGL(push_copy_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s->stream, s->om + (size_t)s->rank * n,
                               (const unsigned long long*)(s->tab_all + 2 * MAX_SEG), s->world, s->rank, (uint64_t)s->rank * n, n);
            HIPCK(hipGetLastError());
        }
        CK(push_barrier(g));
    } else if (g.rccl) {
        if (s0->world > 1 || s0->comm)
            NCCLCK(g_rccl.AllGather(s0->om + (size_t)s0->rank * 2 * s0->n_local, s0->om, (size_t)2 * s0->n_local, ncclDouble, s0->comm, s0->stream));
    } else if (g.R > 1) {
        CK(group_sync(g));
        const size_t blk = (size_t)2 * s0->n_local;
        for (int r = 0; r < g.R; ++r)
            for (int o = 0; o < g.R; ++o)
                if (o != r)
                    HIPCK(hipMemcpyAsync(g.h[o]->om + (size_t)r * blk, g.h[r]->om + (size_t)r * blk, blk * sizeof(double), hipMemcpyDeviceToDevice,
                                         g.h[r]->stream));
        CK(group_sync(g));
    }
    // np.percentile(omega, [25, 75]): position q (N - 1) / 100, the two order statistics around it and the fraction between them
    SelRanks R;
    double tq[2];
    for (int i = 0; i < 2; ++i) {
        const double pos = (i == 0 ? 25.0 : 75.0) / 100.0 * (double)(N - 1);
        const uint32_t lo = (uint32_t)std::floor(pos);
        R.k[2 * i] = lo;
        R.k[2 * i + 1] = std::min(lo + 1u, N - 1u);
        tq[i] = pos - (double)lo;
    }
    for (int r = 0; r < g.R; ++r) {
        bpm_sampler* s = g.h[r];
        launch_outlier_select(s, R);
        HIPCK(hipMemsetAsync(s->olist, 0, sizeof(uint32_t), s->stream));
        hipLaunchKernelGGL(outlier_reset_kernel, dim3((N + WAVE - 1) / WAVE), dim3(WAVE), 0, s->stream, s->L, N, s->lo, s->om, s->sel, tq[0], tq[1],
                           s->ll, s->llhist, (uint32_t)s->hist_rows, s->okeys_ll ? (const PermKey*)(s->okeys + s->okeys_cap) : (const PermKey*)nullptr,
                           s->olist, s->counters + 4);
        hipLaunchKernelGGL(outlier_rebuild_kernel, dim3(std::min<uint32_t>(s->n_local, 4096u)), dim3(WAVE), 0, s->stream, s->L, (const double*)s->sel,
                           (const uint32_t*)s->olist, s->hist, (uint32_t)s->hist_rows, s->okeys_x ? (const PermKey*)s->okeys : (const PermKey*)nullptr,
                           s->w_rows == s->rows_logical ? s->w_mean : (double*)nullptr, s->w_m2);
        HIPCK(hipGetLastError());
        if (local_serial(g)) HIPCK(hipStreamSynchronize(s->stream));
    }
    // (a reset rewrites rows of the generation just appended: its population sums follow)
    for (int r = 0; r < g.R; ++r) CK(push_gen_sums(g.h[r], g.h[r]->rows_logical - 1));
    // push exchange: nobody starts the next generation (whose accepted rows land in THIS replica) while a reset kernel still writes
    if (s0->push_active) CK(push_barrier(g));
    return 0;
}

// demc.py:93-94,116-117: every rank's block into every replica
static int exchange_dense(const Group& g) {
    if (g.rccl) return allgather_state(g.h[0]);
    if (g.R == 1) return 0;
    CK(group_sync(g));
    const bpm_sampler* s0 = g.h[0];
    for (int r = 0; r < g.R; ++r)
        for (int o = 0; o < g.R; ++o)
            if (o != r)
                HIPCK(hipMemcpyAsync(g.h[o]->G + (uint64_t)r * s0->L.blk, g.h[r]->G + (uint64_t)r * s0->L.blk,
                                     (size_t)s0->L.blk * sizeof(double), hipMemcpyDeviceToDevice, g.h[r]->stream));
    return group_sync(g);
}

// the same exchange with only the accepted rows: all-gather of the packed blocks, then scatter into the replicas
static int exchange_sparse(const Group& g) {
    bpm_sampler* s0 = g.h[0];
    const uint32_t cap = s0->xcap;
    const uint64_t S = (uint64_t)s0->xnsub * s0->xstride();
    if (g.rccl) {
        NCCLCK(g_rccl.AllGather(s0->PK + (uint64_t)s0->rank * S, s0->PK, (size_t)S, ncclDouble, s0->comm, s0->stream));
    } else {
        CK(group_sync(g));
        for (int r = 0; r < g.R; ++r)
            for (int o = 0; o < g.R; ++o)
                if (o != r)
                    HIPCK(hipMemcpyAsync(g.h[o]->PK + (uint64_t)r * S, g.h[r]->PK + (uint64_t)r * S, (size_t)S * sizeof(double),
                                         hipMemcpyDeviceToDevice, g.h[r]->stream));
        CK(group_sync(g));
    }
    for (int r = 0; r < g.R; ++r) {
        bpm_sampler* s = g.h[r];
        hipLaunchKernelGGL(exchange_scatter_kernel, dim3(cap * s->xnsub, s->world), dim3(WAVE), 0, s->stream, s->L, s->PK, s->xnsub,
                           s->xstride(), cap, s->rank, s->xstat);
        if (local_serial(g)) HIPCK(hipStreamSynchronize(s->stream));
    }
    HIPCK(hipGetLastError());
    return 0;
}

static void launch_replay_any(bpm_sampler* s, const PhaseArgs& a) {
    const int v = s->cfg.algo != BPM_ALGO_DREAM ? 0 : (s->cfg.del_pairs == 3 ? 1 : 2);
    if (a.rec_sorted && s->shape.idx >= 3 && s->shape.idx < SHAPE_WIDE) g_replay_sorted[v][s->shape.idx - 3](a, s->stream);
    else g_replay[v][s->shape.idx](a, s->stream);
}

// demc.py:93-94,116-117 with one byte per local chain on the wire: all-gather of the accept bytes, then every rank
// recomputes the accepted updates of the other ranks' chains of this half generation into its replica
static int exchange_replay(const Group& g, int ph) {
    bpm_sampler* s0 = g.h[0];
    if (g.rccl) {
        NCCLCK(g_rccl.AllGather(s0->accbits_all + (uint64_t)s0->rank * s0->n_local, s0->accbits_all, (size_t)s0->n_local, ncclUint8,
                                s0->comm, s0->stream));
    } else if (g.R > 1) {
        CK(group_sync(g));
        for (int r = 0; r < g.R; ++r)
            for (int o = 0; o < g.R; ++o)
                if (o != r)
                    HIPCK(hipMemcpyAsync(g.h[o]->accbits_all + (uint64_t)r * s0->n_local, g.h[r]->accbits_all + (uint64_t)r * s0->n_local,
                                         (size_t)s0->n_local, hipMemcpyDeviceToDevice, g.h[r]->stream));
        CK(group_sync(g));
    }
    for (int r = 0; r < g.R; ++r) {
        bpm_sampler* s = g.h[r];
        if (s->world == 1) continue;                        // (one-rank communicator: nobody else's chains)
        PhaseArgs a = s->cur_args[ph];
        if (a.n_upd == 0) continue;
        a.replay = 1u;
        a.accbits = nullptr;
        a.accbits_all = s->accbits_all;
        trace_set(a, nullptr, nullptr, nullptr);
        a.pack = nullptr; a.hist_row = nullptr; a.llhist_row = nullptr; a.adapt_on = 0u;
        launch_replay_any(s, a);
        if (local_serial(g)) HIPCK(hipStreamSynchronize(s->stream));
    }
    HIPCK(hipGetLastError());
    return 0;
}

// xmode: how the half generations' updates reach the other ranks: 0 dense all-gather, 1 accepted rows, 2 accept bytes + replay,
// 3 pushed by their owners from inside the update kernel (then only the cross-rank barrier follows a half generation)
static int group_generation(const Group& g, int64_t n_ahead, int xmode) {
    Dispatch& d = g_disp;
    const long long tp0 = g_host_timing ? now_ns() : 0;
    for (int r = 0; r < g.R; ++r) {
        g.h[r]->sparse_active = xmode == 1;
        g.h[r]->replay_active = xmode == 2;
        g.h[r]->push_active = xmode == 3;
        bind_rank_queue(g.h[r]);
        CK(prepare_generation(g.h[r], n_ahead));
    }
    if (g_host_timing) g_ns_prepare += now_ns() - tp0;
    if (g.h[0]->cfg.algo == BPM_ALGO_DEMC_SYNC) {
        for (int r = 0; r < g.R; ++r) {
            bpm_sampler* s = g.h[r];
            launch_update(s, 0);
            HIPCK(hipMemcpyAsync(s->G + (uint64_t)s->rank * s->L.blk, s->x_next, (size_t)s->n_local * s->ld * sizeof(double),
                                 hipMemcpyDeviceToDevice, s->stream));      // apply the banked updates
        }
        HIPCK(hipGetLastError());
        CK(exchange_dense(g));
    } else {
        for (int ph = 0; ph < 2; ++ph) {
            for (int r = 0; r < g.R; ++r) {
                bpm_sampler* s = g.h[r];
                bind_rank_queue(s);
                if (s->cur_args[ph].n_items > 0) {
                    const bool last_update = ph == 1 || s->cur_args[1].n_items == 0;      // this rank's last update dispatch of the generation
                    d.release_this = d.dq && d.dq_call_last_gen && last_update;
                    if (d.dq && s->timed_last_gen >= 0) {
                        // direct mode: attaching a time stamp costs the host nothing -- the first and the last update dispatch of the call
                        if (s->timed_want_first) { s->timed_want_first = false; d.sig = 0; s->timed_l0 = d.timed_launches; }
                        else if (s->timed_last_gen == s->t_abs && last_update) { d.sig = 1; s->timed_l1 = d.timed_launches; }
                    } else if (s->timed_want_first && s->timed_skip > 0) {
                        --s->timed_skip;
                    } else if (s->timed_want_first) {
                        s->timed_want_first = false; d.stop_event = s->ev0; s->timed_l0 = d.timed_launches;
                    } else if (s->timed_last_gen == s->t_abs && last_update) {
                        d.stop_event = s->ev1; s->timed_l1 = d.timed_launches;
                    }
                    const long long tl0 = g_host_timing ? now_ns() : 0;
                    launch_update(s, ph);
                    if (g_host_timing) { const long long tl1 = now_ns(); g_ns_launch += tl1 - tl0; ++g_n_launch; if (s->timed_last_gen >= 0) { g_launch_log.push_back(tl0); g_launch_log.push_back(tl1); } }
                }
                if (local_serial(g)) HIPCK(hipStreamSynchronize(g.h[r]->stream));
            }
            HIPCK(hipGetLastError());
            CK(xmode == 3 ? push_barrier(g) : (xmode == 2 ? exchange_replay(g, ph) : (xmode == 1 ? exchange_sparse(g) : exchange_dense(g))));
        }
    }
    for (int r = 0; r < g.R; ++r) { bind_rank_queue(g.h[r]); CK(finish_generation(g.h[r])); }
    // push exchange during CR adaptation: the next generation's updates write their (delta, cr) slots into every replica; no rank may
    // get there while another rank's reduction kernels still read this generation's slots
    if (xmode == 3 && g.h[0]->gen_cr_reduce) CK(push_barrier(g));
    if (g.h[0]->outlier_due) {
        // everything of the check, its cross-rank barriers included, runs on the HIP streams: queues drained before, streams after
        std::vector<StreamSection> secs;
        for (int r = 0; r < (d.group_direct ? g.R : 1); ++r) { bind_rank_queue(g.h[r]); secs.emplace_back(g.h[r]); CK(secs.back().rc); }
        {
            OnHipStream on_stream;
            CK(group_outlier_check(g));
        }
        for (auto& sec : secs) CK(sec.end());
    }
    return 0;
}

struct HostCkpt {
    int64_t k_gen, t_abs, hist_rows, rows_logical, w_rows;
};

// Does this group's generation loop go through the library's own AQL queue(s)?  A single GPU's sampler, or -- with the push exchange, where
// nothing of the loop is a collective call -- a rank of a world; group_direct: the R ranks of a local group, each on a queue of its own.
// (run_generations and the arena self-test of bpm_push_selftest ask the same question: the probe must take the path the updates take.)
static bool group_goes_direct(const Group& g, bool push, bool& group_direct) {
    bpm_sampler* s0 = g.h[0];
    group_direct = push && g.R > 1 && !g_host_timing && !local_serial(g);
    for (int r = 0; r < g.R && group_direct; ++r)
        group_direct = g.h[r]->dq_private && g.h[r]->dq_enabled && !g.h[r]->dq->failed() && !g.h[r]->trace_i32 && !g.h[r]->stamps && !g.h[r]->shape_needs_scratch;
    return group_direct ||
           (s0->dq && s0->dq_enabled && g.R == 1 && ((!g.rccl && s0->world == 1) || push) && (!s0->local_group || s0->dq_private) &&
            s0->cfg.algo != BPM_ALGO_DEMC_SYNC && !s0->trace_i32 && !s0->stamps && !g_host_timing && !s0->dq->failed() && !s0->shape_needs_scratch);
}

static int run_generations_user(bpm_sampler* s, int64_t n_gens);      // (a host-callback sampler with a device likelihood: below, beside the host-callback core)
// the update kernel compiled at run time around a caller's likelihood (bpm_sampler::like.fused): the general instantiation's launch, from a module
static void launch_user_fused(const PhaseArgs& a, int flavour, hipStream_t st) {
    Dispatch& d = g_disp;
    bpm_sampler* s = d.user_cur;
    if (!s || !s->like.fused.fn) { d.user_launch_failed = true; return; }      // (never: run_generations routes here only with the module in place -- and says so if not)
    PhaseArgs ka = a;
    ka.tparams = s->like.params.p;                   // the caller's parameter block is the target's
    // [0] the general instantiation, [1] the steady-state one, [2] the burn-in one: prepare_generation chose among those the module holds
    const UserLikelihood::Fused& m = s->like.fused;
    const int k = hot_is_adapt(flavour) ? 2 : (flavour_is_steady(flavour) ? 1 : 0);
    const unsigned block = k == 2 ? m.block_adapt : m.block, cpw = block / (unsigned)s->shape.lpc, grid = (a.n_items + cpw - 1u) / cpw;
    // (launch_packed's two paths; the module's kernels take the argument block alone, no preloaded leading arguments)
    if (d.dq) return update_packet(d, d.dq->kernel_by_name(m.names[k]), grid, block, &ka, sizeof(ka));
    update_on_stream(d, k == 2 ? m.adapt : (k == 1 ? m.hot : m.fn), grid, block, &ka, sizeof(ka), st);
}
static int run_generations(const Group& g, int64_t n_gens) {
    bpm_sampler* s0 = g.h[0];
    // a caller's likelihood compiled from HIP source (bpm_set_device_likelihood): the update kernel compiled around it runs the ordinary generation loop
    // (one launch per half generation, on the HIP stream); without it, the proposal / likelihood / commit kernels of run_generations_user
    const bool user_fused = s0->cfg.target_id == BPM_TARGET_HOST_CALLBACK && s0->like.fused.fn != nullptr && g.R == 1;
    if (s0->cfg.target_id == BPM_TARGET_HOST_CALLBACK && s0->like.fn && g.R == 1 && !user_fused) return run_generations_user(s0, n_gens);
    if (user_fused && s0->world > 1 && !s0->comm) return fail("bpm_step: a host-callback sampler of a world needs an RCCL communicator (create it with a unique id)");
    if (!user_fused && !pick_fused(s0)) return fail("bpm_step: host-callback target must be driven with bpm_propose / bpm_commit (or give it a device likelihood: bpm_set_device_likelihood)");
    const bool dream = s0->cfg.algo == BPM_ALGO_DREAM;
    int64_t done = 0;
    const bool push = s0->push_enabled && s0->push_connected;
    if (s0->world > 1 && !push && !g.rccl && g.R == 1) return fail("bpm_step: this rank has no exchange yet: call bpm_push_connect (and bpm_set_exchange(h, 3, 0)) on every rank first");
    bool push_entered = false;
    while (done < n_gens) {
        const bool adapting = dream && s0->cfg.burnin_gen > s0->k_gen;          // dream.py:92: CR statistics travel in the dense block
        // one generation, or one chunk of generations under the sparse exchange (prepare_generation asks Dispatch::user_cur who drives a host-callback sampler)
        DispatchScope scope(user_fused ? s0 : nullptr);
        Dispatch& d = scope.d;
        if (push || !(s0->sparse_enabled && !adapting)) {
            // (HIP-graph replay of steady-state chunks was built and measured in round 1 -- 13.1 vs 12.5 us per generation at cfg2 -- and
            // removed in round 3: DESIGN.md section 5 item 6)
            const bool replay = s0->replay_enabled && !adapting;       // burn-in: delta / cr_idx of every chain travel in the dense block
            // Direct mode: a single GPU's generation loop (the two update kernels, during burn-in the CR reduction, once per window
            // the table build) is dispatched through the library's own AQL queue.  The outlier check and the moment rebuild (rare) run
            // on the HIP stream between two drains (StreamSection); the synchronous mode, tracing and everything with an exchange
            // stay on the stream altogether.
            // With the push exchange a rank of a world runs on its own queue too: nothing of its generation loop is a collective call.
            bool group_direct = false;
            // (a run-time module's kernels go through the library's queue when it found them by name, else on the stream)
            const bool direct = group_goes_direct(g, push, group_direct) && (!user_fused || s0->like.fused.dq);
            for (int r = 0; r < g.R; ++r) {
                bpm_sampler* s = g.h[r];
                if (direct && !s->dq_active) {
                    CK(wait_stream(s->stream));                         // what the stream still holds (burn-in, table builds) comes first
                    s->dq_active = true;
                    d.mark_acquire(true);
                } else if (!direct && s->dq_active) {
                    CK(leave_direct(s));
                }
            }
            d.group_direct = group_direct;
            d.dq = direct ? s0->dq : nullptr;
            // (half a generation rewrites at most N/2 + 1 rows)
            // Release-less packets + write-through stores in every generation, burn-in included, at every size: with ONE 16-byte sc1 store
            // per lane (store_row_wt16) the write-through form beats the end-of-kernel release everywhere it was measured -- round 2's two
            // 8-byte atomic stores lost above 4 MiB per half generation and in burn-in, hence its size rule and the fenced burn-in
            // (profiles/r03_write_through_16B.txt: cfg2 burn-in 23.1 -> 21.9 us, cfg5 57.6 -> 55.9, cfg5 burn-in 90 -> 81, N = 65536 x d = 100 70.0 -> 68.7).
            // BPM_TEST_PATHS=wt8 selects the 8-byte form, bpm_set_launch_path(h, 1, 3) the fenced packets with plain stores.
            d.update_fence = s0->dq_fence;
            // push exchange: system scope -- every update packet acquires and releases at SYSTEM scope, plain stores into the own replica (rows
            // go to and come from other agents); agent scope -- the single-GPU form: acquire only, write-through stores into the own replica
            if (push && !s0->push_agent_scope) d.update_fence = bpm::DirectQueue::FENCED | bpm::DirectQueue::SYSTEM;
            d.wt_stores = !s0->coherent && direct && !(d.update_fence & bpm::DirectQueue::RELEASE);
            d.dq_call_last_gen = direct && done == n_gens - 1;
            d.call_last_gen = done == n_gens - 1;
            if (push && !push_entered) {
                // entry barrier of the call: a peer's first update kernel may push into THIS replica only after this rank has finished
                // whatever its host did to the replica before the call (bpm_set_state, a warm start, ...) -- and vice versa
                for (int r = 0; r < g.R; ++r) g.h[r]->push_active = true;
                CK(push_barrier(g));
                push_entered = true;
            }
            const int rc_gen = group_generation(g, n_gens - done, push ? 3 : (replay ? 2 : 0));
            if (direct) {
                for (int r = 0; r < (group_direct ? g.R : 1); ++r) {
                    bpm_sampler* s = g.h[r];
                    s->dq->flush();                                     // one doorbell per generation
                    if (d.dq_error || s->dq->failed()) return fail("direct AQL queue: " + (s->dq->why().empty() ? std::string("update kernel not found among the loaded code objects") : s->dq->why()));
                }
            }
            CK(rc_gen);
            if (d.user_launch_failed) return fail("bpm_step: the update kernel compiled around the HIP-source likelihood was not launched (module gone)");
            if (push) for (int r = 0; r < g.R; ++r) g.h[r]->n_push_gens += 1;
            else if (replay) for (int r = 0; r < g.R; ++r) g.h[r]->n_replay_gens += 1;
            ++done;
            continue;
        }
        // ---- a chunk of generations with the sparse exchange, under a checkpoint
        const int64_t K = std::min<int64_t>(SPARSE_CHUNK, n_gens - done);
        std::vector<HostCkpt> hc((size_t)g.R);
        for (int r = 0; r < g.R; ++r) {
            bpm_sampler* s = g.h[r];
            hc[(size_t)r] = HostCkpt{s->k_gen, s->t_abs, s->hist_rows, s->rows_logical, s->w_rows};
            HIPCK(hipMemcpyAsync(s->ckpt_G, s->G, (size_t)s->world * s->L.blk * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
            HIPCK(hipMemcpyAsync(s->ckpt_ll, s->ll, (size_t)s->n_local * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
            HIPCK(hipMemcpyAsync(s->ckpt_acc, s->acc_count, ((size_t)s->n_local + ACC_SHARDS) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s->stream));
            HIPCK(hipMemcpyAsync(s->ckpt_counters, s->counters, 4 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s->stream));
            HIPCK(hipMemsetAsync(s->xstat, 0, 2 * sizeof(uint32_t), s->stream));
            for (uint32_t b = 0; b < s->xnsub; ++b)      // own counters armed (the capacity, hence the layout, may have changed)
                HIPCK(hipMemsetAsync(s->PK + ((uint64_t)s->rank * s->xnsub + b) * s->xstride(), 0, sizeof(double), s->stream));
        }
        for (int64_t i = 0; i < K; ++i) CK(group_generation(g, n_gens - done - i, 1));
        bool overflow = false;
        uint32_t maxc = 0;
        for (int r = 0; r < g.R; ++r) {
            bpm_sampler* s = g.h[r];
            uint32_t xs[2] = {0, 0};
            HIPCK(hipMemcpyAsync(xs, s->xstat, sizeof(xs), hipMemcpyDeviceToHost, s->stream));
            HIPCK(hipStreamSynchronize(s->stream));
            overflow = overflow || xs[0] != 0;
            maxc = std::max(maxc, xs[1]);
            s->n_sparse_chunks += 1;
        }
        if (overflow) {
            // some rank accepted more rows than a packed block holds: replicas diverged.  Roll every rank back to the
            // checkpoint and replay the chunk with the dense exchange; the draws are counter-addressed, so the replay
            // is exactly the run that would have happened without the sparse exchange.
            for (int r = 0; r < g.R; ++r) {
                bpm_sampler* s = g.h[r];
                HIPCK(hipMemcpyAsync(s->G, s->ckpt_G, (size_t)s->world * s->L.blk * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
                HIPCK(hipMemcpyAsync(s->ll, s->ckpt_ll, (size_t)s->n_local * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
                HIPCK(hipMemcpyAsync(s->acc_count, s->ckpt_acc, ((size_t)s->n_local + ACC_SHARDS) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s->stream));
                HIPCK(hipMemcpyAsync(s->counters, s->ckpt_counters, 4 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s->stream));
                const HostCkpt& k = hc[(size_t)r];
                s->k_gen = k.k_gen; s->t_abs = k.t_abs; s->hist_rows = k.hist_rows; s->rows_logical = k.rows_logical; s->w_rows = k.w_rows;
                s->n_sparse_replays += 1;
            }
            for (int64_t i = 0; i < K; ++i) CK(group_generation(g, n_gens - done - i, 0));
        }
        // capacity for the next chunk from the largest sub-block count seen (identical on every rank: all see all
        // counters): a margin of ~3 sigma of a Poisson count on top of an observed maximum over >= 64 half generations
        const uint32_t want = overflow ? 2u * maxc + 8u : maxc + 3u * (uint32_t)std::ceil(std::sqrt((double)maxc)) + 4u;
        for (int r = 0; r < g.R; ++r) {
            bpm_sampler* s = g.h[r];
            s->xcap = std::min<uint32_t>(s->xcap_max, (want + 1u) & ~1u);
        }
        done += K;
    }
    for (int r = 0; r < g.R; ++r) { g.h[r]->sparse_active = false; g.h[r]->replay_active = false; g.h[r]->push_active = false; }
    return 0;
}

#ifdef BPM_TEST_HOOKS
// Lock-step driver of a local group (see bpm_create): handles[r] = rank r of R, all on one GPU.  Test variant only (include/bipymc_hip_test.h).
extern "C" int bpm_local_group_step(bpm_handle_t* handles, int32_t R, int64_t n_gens) {
    if (!handles || R < 1) return fail("bpm_local_group_step: bad argument");
    for (int r = 0; r < R; ++r) {
        bpm_sampler* s = handles[r];
        CK(check_handle(s));
        if (!s->local_group || (int)s->world != R || (int)s->rank != r) return fail("bpm_local_group_step: handles are not ranks 0..R-1 of one local group");
        if (!s->run_open) return fail("bpm_local_group_step: call bpm_begin_run on every rank first");
        if (s->cfg.keep_history) CK(reserve_history(s, stored_rows_after(s, n_gens), "bpm_local_group_step"));
    CK(ensure_gen_sums(s, s->rows_logical + n_gens));
    }
    CK(set_device(handles[0]));
    Group g{handles, R, false};
    CK(run_generations(g, n_gens));
    for (int r = 0; r < R; ++r) CK(leave_direct(handles[r]));      // (ranks with queues of their own: everything is enqueued on all of them by now)
    return group_sync(g);
}
#endif   // BPM_TEST_HOOKS

extern "C" int bpm_step(bpm_handle_t s, int64_t n_gens) {
    CK(check_handle_keep_direct(s));
    CK(set_device(s));
    // (a rank of a local group with a queue of its own and the push exchange is as independent as a process of its own: one host
    // thread per rank may drive it through bpm_step, the ranks then meet in the cross-rank barrier kernels like the ranks of a world)
    if (s->local_group && !(s->dq_private && s->push_connected && s->push_enabled))
        return fail("bpm_step: ranks of a local test group are driven by bpm_local_group_step (test variant)");
    if (!s->run_open) return fail("bpm_step: call bpm_begin_run first");
    if (n_gens < 0) return fail("bpm_step: n_gens < 0");
    if (s->cfg.keep_history) CK(reserve_history(s, stored_rows_after(s, n_gens), "bpm_step"));
    CK(ensure_gen_sums(s, s->rows_logical + n_gens));
    bpm_sampler* one[1] = {s};
    Group g{one, 1, s->comm != nullptr};
    return run_generations(g, n_gens);
}

// Exchange policy of a world_size > 1 sampler.  mode: 2 = accept bytes + replay (default), 1 = accepted rows in packed
// blocks, 0 = dense all-gather; cap > 0 sets the capacity of the next chunk of mode 1 (rows per sub-block per half
// generation; rounded up to even, clamped to [2, all chains of a sub-block]).  The same values on every rank of a world.
extern "C" int bpm_set_exchange(bpm_handle_t s, int32_t mode, int32_t cap) {
    CK(check_handle(s));
    if (mode < 0 || mode > 3) return fail("bpm_set_exchange: mode must be 0 (dense), 1 (rows), 2 (replay) or 3 (push)");
    if (mode == 3 && !s->push_connected) return fail("bpm_set_exchange: the push exchange needs bpm_push_connect first");
    if (mode == 3 && s->push_failed) return fail("bpm_set_exchange: a wait of the push exchange ran into its limit earlier (the ranks' barrier counters no longer agree): this sampler can only go on with an RCCL exchange");
    if (mode != 3 && s->push_no_rccl) return fail("bpm_set_exchange: this sampler was created without an RCCL communicator: the push exchange is its only one");
    if (!s->PK) return mode ? fail("bpm_set_exchange: this sampler only has the dense exchange (world_size 1, synchronous DE-MC or host callback)") : 0;
    if ((mode == 1 || mode == 2) && s->shape.idx == SHAPE_WIDE)
        return fail("bpm_set_exchange: rows wider than 512 coordinates exchange by push (3) or by the dense all-gather (0): the looped kernel has no replay / packed-rows form");
    if (s->push_enabled && mode != 3) s->cur = -1;      // (windows built with this rank's records only are rebuilt: ensure_perm_table)
    if (s->push_failed && mode != 3) {                  // leaving a push exchange that timed out: the next bpm_synchronize must not report it again
        CK(set_device(s));
        HIPCK(hipMemset(&s->ctrl->err, 0, sizeof(unsigned long long)));
    }
    s->push_enabled = mode == 3;
    if (mode == 3) s->push_agent_scope = (cap & 1) != 0;
    s->sparse_enabled = mode == 1;
    s->replay_enabled = mode == 2;
    if (mode == 1 && cap > 0) s->xcap = std::min<uint32_t>(s->xcap_max, ((uint32_t)cap + 1u) & ~1u);
    return 0;
}

// out[0] = mode (0 dense, 1 rows, 2 replay), out[1] = current capacity of mode 1, out[2] = chunks run with mode 1,
// out[3] = chunks of mode 1 replayed dense, out[4] = generations exchanged by replay
extern "C" int bpm_get_exchange_stats(bpm_handle_t s, int64_t* out) {
    CK(check_handle(s));
    if (!out) return fail("bpm_get_exchange_stats: null argument");
    out[0] = (s->push_enabled && s->push_connected) ? 3 : (s->replay_enabled ? 2 : (s->sparse_enabled ? 1 : 0));
    out[1] = (int64_t)s->xcap;
    out[2] = s->n_sparse_chunks;
    out[3] = s->n_sparse_replays;
    out[4] = s->n_replay_gens;
    out[5] = s->n_push_gens;
    // bits 0-1: connected (2: control block fine-grained); bit 2 / 3: the arena self-test passed with system- / agent-scope packet fences;
    // bit 4: it ran on the library's own queue
    out[6] = (s->push_connected ? (s->ctrl_fine ? 2 : 1) : 0) | (s->probe_sys_ok ? 4 : 0) | (s->probe_agent_ok ? 8 : 0) | (s->probe_direct ? 16 : 0);
    out[7] = (int64_t)s->push_seq | (s->push_agent_scope ? (1ll << 62) : 0);
    return 0;
}

// ---- push exchange: connection ---------------------------------------------------------------------------------------------
// What a rank publishes about its arena (bpm_push_export), BPM_PUSH_BLOB_BYTES in all.  The blobs of all ranks, in rank order, are what
// bpm_push_connect takes: the caller moves them with whatever it has (mpi4py allgather, torch.distributed, a file).
struct PushBlob {
    uint64_t magic;
    int64_t pid;
    int32_t rank, world, device, has_ipc;
    uint64_t arena_addr, arena_bytes, off_om, off_ctrl, n_chains, dim;
    hipIpcMemHandle_t handle;
    uint64_t ctrl_addr;            // != 0: the control block is an allocation of its own (fine-grained), exported by ctrl_handle
    hipIpcMemHandle_t ctrl_handle;
};
static_assert(sizeof(PushBlob) <= BPM_PUSH_BLOB_BYTES, "blob size");
static constexpr uint64_t PUSH_MAGIC = 0x4850555350504D42ull;      // "BPMPUSPH"

extern "C" int bpm_push_export(bpm_handle_t s, void* blob) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!blob) return fail("bpm_push_export: null argument");
    if (!s->arena) return fail("bpm_push_export: this sampler has no push exchange (world_size 1, more than 16 ranks, synchronous DE-MC or host callback)");
    PushBlob b;
    std::memset(&b, 0, sizeof(b));
    b.magic = PUSH_MAGIC; b.pid = (int64_t)getpid(); b.rank = (int32_t)s->rank; b.world = (int32_t)s->world; b.device = s->cfg.device;
    b.arena_addr = (uint64_t)(uintptr_t)s->arena; b.arena_bytes = s->arena_bytes; b.off_om = s->off_om; b.off_ctrl = s->off_ctrl;
    b.n_chains = s->N; b.dim = s->dim;
    if (hipIpcGetMemHandle(&b.handle, s->arena) == hipSuccess) b.has_ipc = 1;
    else { (void)hipGetLastError(); b.has_ipc = 0; }      // (ranks of ONE process need no handle; another process will be told)
    if (s->ctrl_fine) {
        b.ctrl_addr = (uint64_t)(uintptr_t)s->ctrl;
        if (hipIpcGetMemHandle(&b.ctrl_handle, s->ctrl) != hipSuccess) { (void)hipGetLastError(); b.has_ipc = 0; }
    }
    std::memset(blob, 0, BPM_PUSH_BLOB_BYTES);
    std::memcpy(blob, &b, sizeof(b));
    return 0;
}

extern "C" int bpm_push_connect(bpm_handle_t s, const void* blobs) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!blobs) return fail("bpm_push_connect: null argument");
    if (!s->arena) return fail("bpm_push_connect: this sampler has no push exchange");
    if (s->push_connected) return fail("bpm_push_connect: already connected");
    HIPCK(hipStreamSynchronize(s->stream));
    std::vector<unsigned long long> all(3 * MAX_SEG, 0ull), others(MAX_PEERS, 0ull);
    uint32_t n_others = 0;
    // (a failure half way leaves nothing mapped: a later attempt starts from scratch)
    struct Undo {
        bpm_sampler* s; bool armed = true;
        ~Undo() {
            if (!armed) return;
            for (uint32_t p = 0; p < (uint32_t)MAX_SEG; ++p) {
                if (s->peer_opened[p] && s->peer_base[p]) (void)hipIpcCloseMemHandle(s->peer_base[p]);
                if (s->peer_ctrl_opened[p] && s->peer_ctrl_base[p]) (void)hipIpcCloseMemHandle(s->peer_ctrl_base[p]);
                s->peer_opened[p] = s->peer_ctrl_opened[p] = false; s->peer_base[p] = s->peer_ctrl_base[p] = nullptr;
            }
        }
    } undo{s};
    for (uint32_t p = 0; p < s->world; ++p) {
        PushBlob b;
        std::memcpy(&b, static_cast<const char*>(blobs) + (size_t)p * BPM_PUSH_BLOB_BYTES, sizeof(b));
        if (b.magic != PUSH_MAGIC || b.rank != (int32_t)p || b.world != (int32_t)s->world)
            return fail("bpm_push_connect: blob " + std::to_string(p) + " is not the export of rank " + std::to_string(p) + " of this world");
        if (b.arena_bytes != s->arena_bytes || b.off_om != s->off_om || b.off_ctrl != s->off_ctrl || b.n_chains != s->N || b.dim != s->dim)
            return fail("bpm_push_connect: rank " + std::to_string(p) + " has another sampler shape");
        void* base = nullptr;
        if (p == s->rank) {
            if (b.arena_addr != (uint64_t)(uintptr_t)s->arena || b.pid != (int64_t)getpid()) return fail("bpm_push_connect: the blob of this rank is not its own export");
            base = s->arena;
        } else if (b.pid == (int64_t)getpid()) {
            base = reinterpret_cast<void*>((uintptr_t)b.arena_addr);          // a rank of the same process (local test group): the pointer itself
        } else {
            if (!b.has_ipc) return fail("bpm_push_connect: rank " + std::to_string(p) + " could not export an IPC handle of its buffer (hipIpcGetMemHandle failed there: on hosts "
                                        "whose driver supports dmabuf IPC only, HSA_ENABLE_IPC_MODE_LEGACY=0 must be in the environment before anything initialises HSA)");
            const hipError_t e = hipIpcOpenMemHandle(&base, b.handle, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(std::string("bpm_push_connect: hipIpcOpenMemHandle of rank ") + std::to_string(p) + "'s buffer failed: " + hipGetErrorString(e) +
                            " (HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment of every rank? peer access between the devices?)");
            }
            s->peer_opened[p] = true;
            s->peer_base[p] = base;
            // what was mapped must be at least as large as the arena the blob describes: a handle of some other, smaller allocation would make
            // the first store beyond its end a GPU memory fault instead of an error here
            void* rb = nullptr; size_t rsz = 0;
            if (hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&rb), &rsz, base) == hipSuccess) {
                const size_t avail = rsz - (size_t)((char*)base - (char*)rb);
                if (avail < s->arena_bytes)
                    return fail("bpm_push_connect: the buffer mapped for rank " + std::to_string(p) + " holds " + std::to_string(avail) + " bytes, its arena needs " +
                                std::to_string(s->arena_bytes) + " (not the handle of that rank's exchange buffer)");
            } else (void)hipGetLastError();
        }
        s->peer_base[p] = base;
        const unsigned long long a = (unsigned long long)(uintptr_t)base;
        unsigned long long ctrl_a = a + s->off_ctrl;
        if (b.ctrl_addr != 0) {                              // the peer keeps its control block in a fine-grained allocation of its own
            void* cb = nullptr;
            if (p == s->rank) cb = s->ctrl;
            else if (b.pid == (int64_t)getpid()) cb = reinterpret_cast<void*>((uintptr_t)b.ctrl_addr);
            else {
                const hipError_t e = hipIpcOpenMemHandle(&cb, b.ctrl_handle, hipIpcMemLazyEnablePeerAccess);
                if (e != hipSuccess) { (void)hipGetLastError(); return fail(std::string("bpm_push_connect: hipIpcOpenMemHandle of rank ") + std::to_string(p) + "'s control block failed: " + hipGetErrorString(e)); }
                s->peer_ctrl_opened[p] = true;
            }
            s->peer_ctrl_base[p] = cb;
            ctrl_a = (unsigned long long)(uintptr_t)cb;
        }
        all[p] = a; all[MAX_SEG + p] = ctrl_a; all[2 * MAX_SEG + p] = a + s->off_om;
        if (p != s->rank) others[n_others++] = a;
    }
    for (uint32_t i = n_others; i < (uint32_t)MAX_PEERS; ++i) others[i] = others[0];
    HIPCK(hipMemcpy(s->tab_all, all.data(), all.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(s->tab_peerG, others.data(), others.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    undo.armed = false;
    s->push_connected = true;
    s->push_enabled = true;               // connected: the default exchange from here on (bpm_set_exchange chooses another)
    return 0;
}

// One launch of push_arena_probe_kernel for rank s (kernels.h): on the library's own queue when the self-test runs there, else on the stream.
static int launch_arena_probe(bpm_sampler* s, int mode, int form, unsigned long long seed, double* save, int fence) {
    ProbeGeo geo{s->L.blk, s->n_local, s->ld, (s->om && s->off_om) ? 2u * s->n_local : 0u, s->world, s->rank, 2u * s->ld + 8u};
    unsigned long long* bad = &s->ctrl->arena_bad[form];
    return launch_side(s->stream, push_arena_probe_kernel, "push_arena_probe_kernel", dim3(PROBE_REGIONS, s->world), WAVE, fence, Then::ACQUIRE, s->tab_all, geo, mode, seed, save, bad);
}

// Collective over the ranks (all processes call it together; a local group passes its R handles), in two parts.
// (1) control blocks: every rank writes a pattern into every other rank's (fine-grained) control block, one cross-rank barrier, every rank checks.
// (2) arenas: every rank stores probe rows into ITS block of every peer's arena -- first and last row, the block's last slots, both ends of its
//     om block: the addresses its update kernels will push to -- FROM THE QUEUE AND UNDER THE PACKET FENCES THE UPDATE KERNELS USE (the library's
//     own AQL queue where the sampler runs on one), a cross-rank barrier, every rank verifies what arrived in its own arena and puts back what
//     was there.  Once with system-scope fences (decides *ok with part 1), once with the agent-scope form (reported by bpm_get_exchange_stats:
//     a caller skips "push with agent-scope fences" when its probe failed).  Round 3 probed the control block only, from the HIP stream: the
//     arena was first touched by real updates.
// *ok = 1: this rank (every rank of the group) received everything its peers sent.
extern "C" int bpm_push_selftest(bpm_handle_t* handles, int32_t R, int32_t* ok) {
    if (!handles || R < 1 || !ok) return fail("bpm_push_selftest: bad argument");
    *ok = 0;
    for (int r = 0; r < R; ++r) {
        bpm_sampler* s = handles[r];
        CK(check_handle(s));
        if (!s->push_connected) return fail("bpm_push_selftest: call bpm_push_connect first");
        if (R > 1 && (!s->local_group || (int)s->world != R || (int)s->rank != r)) return fail("bpm_push_selftest: handles are not ranks 0..R-1 of one local group");
    }
    CK(set_device(handles[0]));
    Group g{handles, R, false};
    const unsigned long long seed = 0xB1900000ull + handles[0]->push_seq;
    for (int r = 0; r < R; ++r) {
        bpm_sampler* s = handles[r];
        HIPCK(hipMemsetAsync(&s->ctrl->arena_bad[0], 0, 2 * sizeof(unsigned long long), s->stream));
        hipLaunchKernelGGL(push_probe_kernel, dim3(1), dim3(WAVE), 0, s->stream, (const unsigned long long*)(s->tab_all + MAX_SEG), s->world, s->rank, seed);
        HIPCK(hipGetLastError());
    }
    CK(push_barrier(g));
    CK(group_sync(g));
    bool ctrl_ok = true;
    for (int r = 0; r < R; ++r) {
        bpm_sampler* s = handles[r];
        PushCtrl c;
        HIPCK(hipMemcpy(&c, s->ctrl, sizeof(c), hipMemcpyDeviceToHost));
        if (c.err != 0) ctrl_ok = false;
        for (uint32_t p = 0; p < s->world; ++p)
            if (p != s->rank && c.probe[p] != seed + p) ctrl_ok = false;
    }
    // ---- part 2: the arenas, on the path the update kernels take
    std::vector<DevTemp<double>> save((size_t)R);
    for (int r = 0; r < R; ++r) CK(save[(size_t)r].alloc((size_t)handles[r]->world * (2 * handles[r]->ld + 8)));
    bool group_direct = false;
    const bool direct = group_goes_direct(g, true, group_direct);
    for (int r = 0; r < R; ++r) {
        bpm_sampler* s = handles[r];
        if (direct && !s->dq_active) { CK(wait_stream(s->stream)); s->dq_active = true; }
    }
    int rc = 0;
    {   // the probes go where the update kernels would: the dispatch state of a generation, for the length of this block
        DispatchScope scope;
        Dispatch& d = scope.d;
        d.group_direct = group_direct;
        d.dq = direct ? handles[0]->dq : nullptr;
        d.mark_acquire(true);
        for (int form = 0; form < 2 && rc == 0; ++form) {
            // form 0: acquire + release at system scope around the writer (what the HSA memory model asks for between agents); form 1: the single-GPU
            // form, acquire only at agent scope -- the probe rows themselves are system-scope write-through stores either way, as the pushed rows are
            const int f_read = form == 0 ? (bpm::DirectQueue::ACQUIRE | bpm::DirectQueue::SYSTEM) : bpm::DirectQueue::ACQUIRE;
            const int f_write = form == 0 ? (bpm::DirectQueue::FENCED | bpm::DirectQueue::SYSTEM) : bpm::DirectQueue::ACQUIRE;
            for (int mode = 0; mode < 3 && rc == 0; ++mode) {
                rc = push_barrier(g);
                for (int r = 0; r < R && rc == 0; ++r) {
                    bind_rank_queue(handles[r]);
                    rc = launch_arena_probe(handles[r], mode, form, seed + 16u * (unsigned)form, save[(size_t)r].p, mode == 1 ? f_write : f_read);
                    if (d.dq) d.dq->flush();
                }
            }
            if (rc == 0) rc = push_barrier(g);      // nobody goes on (to the next form, to a generation) while a peer still verifies
        }
    }
    for (int r = 0; r < R; ++r) { const int rl = leave_direct(handles[r]); if (rc == 0) rc = rl; }
    CK(rc);
    CK(group_sync(g));
    bool sys_ok = true, agent_ok = true;
    for (int r = 0; r < R; ++r) {
        bpm_sampler* s = handles[r];
        PushCtrl c;
        HIPCK(hipMemcpy(&c, s->ctrl, sizeof(c), hipMemcpyDeviceToHost));
        if (c.err != 0) { sys_ok = false; agent_ok = false; }
        if (c.arena_bad[0] != 0) sys_ok = false;
        if (c.arena_bad[1] != 0) agent_ok = false;
    }
    for (int r = 0; r < R; ++r) { handles[r]->probe_sys_ok = sys_ok; handles[r]->probe_agent_ok = agent_ok; handles[r]->probe_direct = direct; }
    *ok = (ctrl_ok && sys_ok) ? 1 : 0;
    return 0;
}

extern "C" int bpm_get_launch_stats(bpm_handle_t s, int64_t* out) {
    CK(check_handle_keep_direct(s));
    if (!out) return fail("bpm_get_launch_stats: null argument");
    out[0] = s->dq != nullptr ? 1 : 0;
    out[1] = g_disp.n_direct;
    out[2] = g_disp.n_stream;
    out[3] = s->dq_active ? 1 : 0;
    out[4] = s->coherent ? 1 : 0;
    out[5] = s->dq_fence;
    return 0;
}

#ifdef BPM_TEST_HOOKS
// Test hook: the probe behind the choice of packet fences, on the memory type the state would use (coherent_alloc != 0) or on
// ordinary device memory.  *wrong = elements that missed an update (0 = coherent without a release fence), -1 = could not run.
extern "C" int bpm_debug_coherence_probe(int32_t device, int32_t coherent_alloc, int64_t* wrong) {
    if (!wrong) return fail("bpm_debug_coherence_probe: null argument");
    HIPCK(hipSetDevice(device));
    bpm::DirectQueue* dq = bpm::DirectQueue::for_device(device);
    *wrong = -1;
    if (!dq) return 0;
#ifndef BPM_EXPERIMENT_COHERENT
    if (coherent_alloc != 0) return fail("bpm_debug_coherence_probe: the hardware-coherent memory type is not compiled into this library (experiment build only)");
#endif
    *wrong = coherence_probe(dq, coherent_alloc != 0);
    return 0;
}
#endif   // BPM_TEST_HOOKS

extern "C" int bpm_set_launch_path(bpm_handle_t s, int32_t direct, int32_t fence) {
    CK(check_handle(s));
    if (fence != -1 && fence != 0 && fence != 1 && fence != 3) return fail("bpm_set_launch_path: fence must be -1 (keep), 0 (none), 1 (acquire) or 3 (acquire + release)");
    if (fence == 0 && !s->coherent) return fail("bpm_set_launch_path: packets without an acquire fence are not available in this library");
    if (fence == 1 && (!s->dq || !s->dq->has_fence_kernel())) return fail("bpm_set_launch_path: acquire-only packets need the library's queue and its fence kernel");
    s->dq_enabled = direct != 0;
    if (fence >= 0) s->dq_fence = fence;
    return 0;
}

extern "C" int bpm_get_step_time(bpm_handle_t s, float* elapsed_ms, int64_t* n_launches);
extern "C" int bpm_step_timed(bpm_handle_t s, int64_t n_gens, float* elapsed_ms, int64_t* n_launches) {
    CK(check_handle_keep_direct(s));
    CK(set_device(s));
    if (s->cfg.algo == BPM_ALGO_DEMC_SYNC) return fail("bpm_step_timed: not available for the synchronous DE-MC mode");
    if (s->cfg.keep_history) CK(reserve_history(s, stored_rows_after(s, n_gens), "bpm_step_timed"));
    CK(ensure_gen_sums(s, s->rows_logical + n_gens));
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (n_launches) *n_launches = 0;
    s->timed_want_first = n_gens > 0;
    // An event-bound dispatch costs the host 10-30 us instead of 2.5.  At the head of a call that starts from an idle GPU this is time
    // the GPU waits; a quarter into the call the host is far enough ahead to absorb it.  So ev0 rides on launch number n/4 (the
    // interval then covers the last three quarters of the call's launches), ev1 on the last one.
    s->timed_skip = n_gens >= 8 ? (2 * n_gens) / 4 : 0;
    s->timed_last_gen = n_gens > 0 ? s->t_abs + n_gens - 1 : -1;
    s->timed_l0 = s->timed_l1 = -1;
    g_launch_log.clear();
    const long long tt0 = g_host_timing ? now_ns() : 0;
    const int rc = bpm_step(s, n_gens);
    s->timed_want_first = false;
    s->timed_last_gen = -1;      // (the riders of the timed launches went with run_generations's scopes)
    CK(rc);
    s->timed_direct = s->dq_active;
    if (s->dq_active) { if (s->dq->drain() != 0) return fail("direct AQL queue: " + s->dq->why()); }     // (the sampler stays in direct mode: the next call goes on)
    else CK(wait_stream(s->stream));
    if (g_host_timing && !g_launch_log.empty() && g_launch_log.size() <= 400) {
        const long long tt1 = now_ns();
        fprintf(stderr, "[bpm host timing] bpm_step_timed(%lld): entry -> drained %.1f us; launch calls (start offset us : duration us):", (long long)n_gens, (tt1 - tt0) * 1e-3);
        for (size_t i = 0; i + 1 < g_launch_log.size(); i += 2)
            fprintf(stderr, " %.1f:%.1f", (g_launch_log[i] - tt0) * 1e-3, (g_launch_log[i + 1] - g_launch_log[i]) * 1e-3);
        fprintf(stderr, "\n");
    }
    // (reading the two events costs tens of microseconds of host time: left to bpm_get_step_time, outside the caller's own clock)
    if (elapsed_ms || n_launches) return bpm_get_step_time(s, elapsed_ms, n_launches);
    return 0;
}

extern "C" int bpm_get_step_time(bpm_handle_t s, float* elapsed_ms, int64_t* n_launches) {
    CK(check_handle_keep_direct(s));
    CK(set_device(s));
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (n_launches) *n_launches = 0;
    if (s->timed_direct && s->timed_l0 >= 0 && s->timed_l1 > s->timed_l0) {
        double t0 = 0.0, t1 = 0.0;                    // end-of-kernel time stamps of the two dispatches, written by the packet processor
        if (!s->dq || !s->dq->dispatch_end_ns(&t0, &t1)) return fail("bpm_get_step_time: no dispatch time stamps");
        if (elapsed_ms) *elapsed_ms = (float)((t1 - t0) * 1e-6);
        if (n_launches) *n_launches = s->timed_l1 - s->timed_l0;
    } else if (s->timed_l0 >= 0 && s->timed_l1 > s->timed_l0) {
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        if (elapsed_ms) *elapsed_ms = ms;
        if (n_launches) *n_launches = s->timed_l1 - s->timed_l0;
    }
    return 0;
}


#ifdef BPM_TEST_HOOKS
// Same generations as bpm_step, with a HIP event pair on the sampler's stream around every
// update-kernel launch: returns the summed kernel time and the number of launches -- a cross-check of
// the per-launch duration bench.py prices the roofline with (rocprofv3 --kernel-trace gives the same
// figure offline).  Test variant only (include/bipymc_hip_test.h): bench.py runs it outside its timed region.
extern "C" int bpm_step_profiled(bpm_handle_t s, int64_t n_gens, double* kernel_ms_sum, int64_t* n_launches) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->run_open) return fail("bpm_step_profiled: call bpm_begin_run first");
    if (s->cfg.target_id == BPM_TARGET_HOST_CALLBACK) return fail("bpm_step_profiled: device targets only");
    if (s->cfg.algo == BPM_ALGO_DEMC_SYNC) return fail("bpm_step_profiled: not available for the synchronous DE-MC mode");
    if (n_gens <= 0 || n_gens > 4096) return fail("bpm_step_profiled: 1 <= n_gens <= 4096");
    // (this entry point exchanges with the dense RCCL all-gather; a world without a communicator has no exchange here)
    if (s->world > 1 && !s->comm) return fail("bpm_step_profiled: not available for a rank of a world without an RCCL communicator (push exchange only): use bpm_step_timed");
    if (s->cfg.keep_history) CK(reserve_history(s, stored_rows_after(s, n_gens), "bpm_step_profiled"));
    CK(ensure_gen_sums(s, s->rows_logical + n_gens));
    std::vector<hipEvent_t> ev((size_t)n_gens * 4);
    for (auto& e : ev) HIPCK(hipEventCreate(&e));
    s->sparse_active = false;
    s->replay_active = false;
    for (int64_t g = 0; g < n_gens; ++g) {
        CK(prepare_generation(s, n_gens - g));
        for (int ph = 0; ph < 2; ++ph) {
            HIPCK(hipEventRecord(ev[(size_t)g * 4 + 2 * ph], s->stream));
            if (s->cur_args[ph].n_items > 0) launch_update(s, ph);
            HIPCK(hipEventRecord(ev[(size_t)g * 4 + 2 * ph + 1], s->stream));
            CK(allgather_state(s));
        }
        HIPCK(hipGetLastError());
        CK(finish_generation(s));
        if (s->outlier_due) { bpm_sampler* one[1] = {s}; CK(group_outlier_check(Group{one, 1, s->comm != nullptr})); }
    }
    HIPCK(hipStreamSynchronize(s->stream));
    double tot = 0.0;
    for (int64_t i = 0; i < 2 * n_gens; ++i) {
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, ev[(size_t)2 * i], ev[(size_t)2 * i + 1]));
        tot += ms;
    }
    for (auto& e : ev) HIPCK(hipEventDestroy(e));
    if (kernel_ms_sum) *kernel_ms_sum = tot;
    if (n_launches) *n_launches = 2 * n_gens;
    return 0;
}
#endif   // BPM_TEST_HOOKS

// How bpm_set_history leaves a handle, and whatever else fills a history from outside (bpm_derive_history, bpm_rank_history): `rows` rows in chain
// order, the state = the last row with its ln-likes current, no proposals open, a new epoch for whoever remembered the old history
static void history_installed(bpm_sampler* s, int64_t rows) {
    for (int64_t r = 0; r < rows && r < (int64_t)s->hist_tag.size(); ++r) s->hist_tag[(size_t)r] = -1;
    s->hist_rows = rows;
    s->rows_logical = rows;
    s->hist_stride = 1;      // (a row per generation: bpm_set_history_thinned says otherwise afterwards)
    s->w_rows = 0;      // moments are rebuilt from the rows when adaptation next needs them
    s->ll_stale = false;
    s->state_set = true;
    s->phase = 0;
    s->hist_epoch += 1;
}

// Warm start (demc.py:46-51,217-233): install `rows` history rows of this rank's chains
// (hist_local: rows x n_local x dim) and the full current state X (N x dim, = last row of every chain).
// x_is_last_row: the dense contract -- X is the last row, so a single row IS what bpm_set_state leaves; a thinned history's X is the CURRENT state,
// which no stored row need be (bpm_set_history_thinned): every row is installed from hist_local then, the only one included
static int install_history(bpm_sampler* s, const char* who, int64_t rows, const double* hist_local, const double* X, bool x_is_last_row) {
    CK(check_handle(s));
    CK(set_device(s));
    if (rows < 1 || !hist_local || !X) return fail(std::string(who) + ": bad argument");
    if (!s->cfg.keep_history && rows > 1) return fail(std::string(who) + ": sampler keeps no history");
    CK(bpm_set_state(s, X));      // (reset_history: a new hist_epoch, the one row)
    s->hist_stride = 1;           // (a row per generation)
    if (rows > 1 || !x_is_last_row) {
        CK(ensure_history(s, rows));
        HIPCK(hipMemsetAsync(s->hist, 0, (size_t)rows * s->n_local * s->ld * sizeof(double), s->stream));
        HIPCK(hipMemcpy2DAsync(s->hist, s->ld * sizeof(double), hist_local, s->dim * sizeof(double), s->dim * sizeof(double),
                               (size_t)rows * s->n_local, hipMemcpyHostToDevice, s->stream));
        // ln_like of the old rows is not stored in the reference's checkpoint: recompute (device targets) or NaN
        if (s->cfg.target_id != BPM_TARGET_HOST_CALLBACK) {
            (void)launch_eval_target(s, s->hist, (uint32_t)((size_t)rows * s->n_local), s->llhist);
            HIPCK(hipGetLastError());
        } else {
            // host-callback target: the caller supplies the current ln-likes next (bpm_set_loglike fills the last row);
            // the older rows are unknown -- NaN, which the outlier check skips
            std::vector<double> nanv((size_t)rows * s->n_local, std::nan(""));
            HIPCK(hipMemcpyAsync(s->llhist, nanv.data(), nanv.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
            HIPCK(hipStreamSynchronize(s->stream));
        }
        history_installed(s, rows);
        if (s->cfg.running_moments) {      // population sums of every installed row
            CK(ensure_gen_sums(s, rows));
            for (int64_t g = 0; g < rows; ++g) CK(push_gen_sums(s, g, s->hist + (uint64_t)g * s->n_local * s->ld));
        }
        HIPCK(hipStreamSynchronize(s->stream));
    }
    return 0;
}
extern "C" int bpm_set_history(bpm_handle_t s, int64_t rows, const double* hist_local, const double* X) {
    return install_history(s, "bpm_set_history", rows, hist_local, X, true);
}

// param_est (demc.py:235-248) without moving the history: raw moments of this rank's part of the
// super chain (row g*N + i = chain i at generation g) for rows >= n_burn:
// count, sum_j (x - shift_j), sum_j (x - shift_j)^2, shift_j (= chain 0's current state, identical
// on every rank).  Ranks combine the three and finish mean / std(ddof=0) on the host.
extern "C" int bpm_reduce_moments(bpm_handle_t s, int64_t n_burn, double* sum, double* sumsq, double* shift,
                                  int64_t* count) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!sum || !sumsq || !shift || !count) return fail("bpm_reduce_moments: null argument");
    if (n_burn < 0) n_burn = 0;
    if (s->cfg.running_moments && !history_resident(s)) {
        // no resident history: answer from the per-generation population sums -- exact for a burn-in of whole generations
        if (n_burn % s->N != 0)
            return fail("bpm_reduce_moments: without a resident history n_burn must be a multiple of n_chains (whole generations)");
        const int64_t g0 = std::min<int64_t>(n_burn / s->N, s->rows_logical), g1 = s->rows_logical;
        std::vector<double> h(3 * (size_t)s->ld, 0.0);
        HIPCK(hipMemcpyAsync(h.data() + 2 * s->ld, s->gs_shift, s->ld * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        *count = (g1 - g0) * (int64_t)s->n_local;
        if (g1 > g0) {
            DevTemp<double> out;
            CK(out.alloc(2 * (size_t)s->ld));
            hipLaunchKernelGGL(moments_final_kernel, dim3(s->ld), dim3(MOM_THREADS), 0, s->stream, (const double*)(s->gen_sums + (size_t)g0 * 2 * s->ld),
                               (uint32_t)(g1 - g0), s->ld, out.p);
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(h.data(), out.p, 2 * s->ld * sizeof(double), hipMemcpyDeviceToHost, s->stream));
            HIPCK(hipStreamSynchronize(s->stream));
        } else {
            HIPCK(hipStreamSynchronize(s->stream));
        }
        for (uint32_t j = 0; j < s->dim; ++j) { sum[j] = h[j]; sumsq[j] = h[s->ld + j]; shift[j] = h[2 * s->ld + j]; }
        return 0;
    }
    uint64_t m_lo = 0, m_hi = 0;
    CK(super_chain_window(s, n_burn, &m_lo, &m_hi));
    std::vector<double> h(3 * (size_t)s->ld, 0.0);
    HIPCK(hipMemcpyAsync(h.data() + 2 * s->ld, s->G, s->ld * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    *count = (int64_t)(m_hi - m_lo);
    if (m_hi > m_lo) {
        // enough blocks for ~8 per CU (each thread keeps MOM_UNR 16-byte loads in flight), at least 64 rows each
        const uint32_t nb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(2048, (m_hi - m_lo + 63) / 64));
        DevTemp<double> part, out;
        CK(part.alloc((size_t)nb * 2 * s->ld));
        CK(out.alloc(2 * (size_t)s->ld));
        hipLaunchKernelGGL(moments_partial_kernel, dim3(nb), dim3(MOM_THREADS), 0, s->stream, s->hist, m_lo, m_hi, s->ld,
                           s->G, part.p);
        hipLaunchKernelGGL(moments_final_kernel, dim3(s->ld), dim3(MOM_THREADS), 0, s->stream, part.p, nb, s->ld, out.p);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(h.data(), out.p, 2 * s->ld * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
    } else {
        HIPCK(hipStreamSynchronize(s->stream));
    }
    for (uint32_t j = 0; j < s->dim; ++j) { sum[j] = h[j]; sumsq[j] = h[s->ld + j]; shift[j] = h[2 * s->ld + j]; }
    return 0;
}

// ---- convergence diagnostics (diagnostics.h; bipymc_amd/diagnostics.py finishes them) --------------------------------------------------
// Split-chain moments of this rank's chains over history rows [g_lo, g_hi): per coordinate the mean of the 2 n_local half-chain means, the
// sum of their squared deviations from it and the sum of the half-chain variances.  The per-half-chain means stay on the device for
// bpm_diag_autocov.
extern "C" int bpm_diag_split_moments(bpm_handle_t s, int64_t g_lo, int64_t g_hi, double* mean_of_means, double* m2_of_means,
                                      double* sum_of_vars, int64_t* n_half_chains, int64_t* n_draws) {
    CK(check_handle(s));
    CK(set_device(s));
    s->dg_seen.valid = false;
    if (!mean_of_means || !m2_of_means || !sum_of_vars || !n_half_chains || !n_draws) return fail("bpm_diag_split_moments: null argument");
    CK(require_resident_history(s, "bpm_diag_split_moments"));
    if (g_lo < 0 || g_hi < g_lo || g_hi > s->hist_rows) return fail("bpm_diag_split_moments: generation range out of bounds");
    const int64_t n = (g_hi - g_lo) / 2;
    if (n < 4)
        return fail("bpm_diag_split_moments: a window of " + std::to_string((long long)(g_hi - g_lo)) + " history rows gives half-chains of " +
                    std::to_string((long long)n) + " draws; at least 4 are needed");
    if (n >= (int64_t)1 << 31) return fail("bpm_diag_split_moments: window too long");
    CK(normalize_history(s, g_lo, g_hi));
    const uint64_t row_d = (uint64_t)s->n_local * s->ld;
    if (!s->dg_mean) {      // (all three or none)
        DevTemp<double> mean, m2, out;
        CK(mean.alloc(2 * (size_t)row_d));
        CK(m2.alloc(2 * (size_t)row_d));
        CK(out.alloc((size_t)std::max(3, DIAG_T) * s->ld));
        s->dg_mean = s->mem.keep(mean); s->dg_m2 = s->mem.keep(m2); s->dg_out = s->mem.keep(out);
    }
    const uint64_t n_pairs = row_d / 2u;
    hipLaunchKernelGGL(diag_split_moments_kernel, dim3((unsigned)((n_pairs + DIAG_THREADS - 1) / DIAG_THREADS), 2), dim3(DIAG_THREADS), 0, s->stream,
                       (const double*)s->hist, row_d, n_pairs, (uint64_t)g_lo, (uint64_t)(g_hi - n), (uint32_t)n, s->dg_mean, s->dg_m2);
    hipLaunchKernelGGL(diag_means_final_kernel, dim3(s->ld), dim3(DIAG_THREADS), 0, s->stream, (const double*)s->dg_mean, (const double*)s->dg_m2,
                       2u * s->n_local, s->ld, (uint32_t)n, s->dg_out);
    HIPCK(hipGetLastError());
    std::vector<double> h(3 * (size_t)s->ld);
    HIPCK(hipMemcpyAsync(h.data(), s->dg_out, h.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    for (uint32_t k = 0; k < s->dim; ++k) {
        mean_of_means[k] = h[k];
        m2_of_means[k] = h[s->ld + k];
        sum_of_vars[k] = h[2 * (size_t)s->ld + k];
    }
    *n_half_chains = 2 * (int64_t)s->n_local;
    *n_draws = n;
    s->dg_g0 = g_lo; s->dg_g1 = g_hi; s->dg_n = n;
    s->dg_seen.take(s);
    return 0;
}

// sum over this rank's half-chains of c_{j,t} (biased autocovariance about the half-chain's mean), t in [t0, t0 + n_lags):
// out[(t - t0) * dim + k].  Window and means of the last bpm_diag_split_moments call.
extern "C" int bpm_diag_autocov(bpm_handle_t s, int64_t t0, int32_t n_lags, double* out) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!out) return fail("bpm_diag_autocov: null argument");
    CK(s->dg_seen.check(s, "bpm_diag_autocov", "bpm_diag_split_moments"));
    if (t0 < 0 || n_lags < 1 || t0 + n_lags > s->dg_n)
        return fail("bpm_diag_autocov: lags [t0, t0 + n_lags) must lie in [0, n) with n = " + std::to_string((long long)s->dg_n) +
                    " draws per half-chain");
    const uint64_t row_d = (uint64_t)s->n_local * s->ld;
    const uint32_t kw = s->ld <= (uint32_t)DIAG_THREADS ? s->ld : (uint32_t)DIAG_THREADS;
    const uint32_t n_kt = (s->ld + kw - 1) / kw, cpw = DIAG_THREADS / kw;
    const uint32_t n_groups = (s->n_local + cpw - 1) / cpw;      // per half
    // ~768 workgroups in all, what is resident at once (three per CU at this kernel's 138 VGPRs): each walks n_groups / nb column groups
    const uint32_t nb = std::max(1u, std::min(n_groups, 384u / n_kt));
    const size_t part_n = (size_t)2 * nb * DIAG_T * s->ld;
    CK(grow_device(s, &s->dg_part, &s->dg_part_cap, part_n));
    std::vector<double> h((size_t)DIAG_T * s->ld);
    const int64_t r_lo1 = s->dg_g1 - s->dg_n;
    for (int64_t b0 = t0; b0 < t0 + n_lags; b0 += DIAG_T) {
        hipLaunchKernelGGL(diag_autocov_kernel, dim3(nb, n_kt, 2), dim3(DIAG_THREADS), 0, s->stream, (const double*)s->hist, row_d, s->n_local, s->ld,
                           (uint64_t)s->dg_g0, (uint64_t)r_lo1, (uint32_t)s->dg_n, (uint32_t)b0, (const double*)s->dg_mean, kw, cpw, s->dg_part);
        hipLaunchKernelGGL(diag_autocov_final_kernel, dim3((s->ld + DIAG_FIN_K - 1) / DIAG_FIN_K, DIAG_T), dim3(DIAG_THREADS), 0, s->stream,
                           (const double*)s->dg_part, 2 * nb, s->ld, (uint32_t)s->dg_n, s->dg_out);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(h.data(), s->dg_out, h.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        const int64_t nl = std::min<int64_t>(DIAG_T, t0 + n_lags - b0);
        for (int64_t l = 0; l < nl; ++l)
            for (uint32_t k = 0; k < s->dim; ++k) out[(size_t)(b0 - t0 + l) * s->dim + k] = h[(size_t)l * s->ld + k];
    }
    return 0;
}

// ---- posterior quantiles (quantiles.h; bipymc_amd/quantiles.py runs the select) --------------------------------------------------------
// Fixes the window of super-chain rows >= n_burn (param_est's unit, the selection of bpm_reduce_moments: a partial first generation by chain
// index) and returns how many of them this rank holds.  bpm_quantile_histogram then counts over that window while the history is unchanged.
extern "C" int bpm_quantile_begin(bpm_handle_t s, int64_t n_burn, int64_t* count) {
    CK(check_handle(s));
    CK(set_device(s));
    s->qs_seen.valid = false;
    if (!count) return fail("bpm_quantile_begin: null argument");
    CK(require_resident_history(s, "bpm_quantile_begin"));
    CK(super_chain_window(s, n_burn, &s->qs_lo, &s->qs_hi));
    s->qs_seen.take(s);
    *count = (int64_t)(s->qs_hi - s->qs_lo);
    return 0;
}

// n_prefix (coordinate, prefix) slots, sorted by coordinate, prefixes of one coordinate strictly increasing; each a prefix of `prefix_bits`
// bits (0, 8, ..., 56) of the keys.  hist[j * 256 + b]: keys of coordinate prefix_dim[j] in the window whose top bits equal prefixes[j] and
// whose next 8 bits are b; n_nan[j] (may be null): how many of those are NaN.
extern "C" int bpm_quantile_histogram(bpm_handle_t s, int64_t n_prefix, const int32_t* prefix_dim, const uint64_t* prefixes,
                                      int32_t prefix_bits, uint64_t* hist, int64_t* n_nan) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!prefix_dim || !prefixes || !hist) return fail("bpm_quantile_histogram: null argument");
    CK(s->qs_seen.check(s, "bpm_quantile_histogram", "bpm_quantile_begin"));
    if (prefix_bits < 0 || prefix_bits > 56 || prefix_bits % 8 != 0)
        return fail("bpm_quantile_histogram: prefix_bits must be one of 0, 8, ..., 56");
    if (n_prefix < 1 || n_prefix > ((int64_t)1 << 24)) return fail("bpm_quantile_histogram: n_prefix out of range");
    const uint32_t bits = (uint32_t)prefix_bits;
    for (int64_t j = 0; j < n_prefix; ++j) {
        if (prefix_dim[j] < 0 || (uint32_t)prefix_dim[j] >= s->dim) return fail("bpm_quantile_histogram: coordinate out of range");
        if (bits == 0 ? prefixes[j] != 0 : (prefixes[j] >> bits) != 0)
            return fail("bpm_quantile_histogram: a prefix has more than prefix_bits bits");
        if (j > 0 && (prefix_dim[j] < prefix_dim[j - 1] || (prefix_dim[j] == prefix_dim[j - 1] && prefixes[j] <= prefixes[j - 1])))
            return fail("bpm_quantile_histogram: slots must be sorted by coordinate, prefixes of a coordinate strictly increasing");
    }
    // tiles of at most QS_SLOTS slots over at most QS_SLOTS coordinates
    std::vector<uint32_t> tiles;
    for (int64_t j = 0; j < n_prefix;) {
        const int64_t j0 = j;
        const uint32_t k0 = (uint32_t)prefix_dim[j0];
        while (j < n_prefix && j - j0 < QS_SLOTS && (uint32_t)prefix_dim[j] - k0 < (uint32_t)QS_SLOTS) ++j;
        tiles.insert(tiles.end(), {(uint32_t)j0, (uint32_t)(j - j0), k0, (uint32_t)prefix_dim[j - 1] - k0 + 1u});
    }
    const size_t n_tiles = tiles.size() / 4;
    const size_t np = (size_t)n_prefix;
    // qs_buf: [hist np x 256 u64 | n_nan np u64 | prefixes np u64 | tiles n_tiles x 16 B (16-byte aligned) | coordinates np u32]
    const size_t o_nan = np * 256 * 8, o_pv = o_nan + np * 8, o_tiles = (o_pv + np * 8 + 15) / 16 * 16, o_pk = o_tiles + n_tiles * 16,
                 need = o_pk + np * 4;
    CK(grow_device(s, &s->qs_buf, &s->qs_cap, need));
    std::vector<unsigned char> in(need - o_pv);
    std::memcpy(in.data(), prefixes, np * 8);
    std::memcpy(in.data() + (o_tiles - o_pv), tiles.data(), n_tiles * 16);
    stage_dims(in.data() + (o_pk - o_pv), prefix_dim, np);
    HIPCK(hipMemsetAsync(s->qs_buf, 0, o_pv, s->stream));
    HIPCK(hipMemcpyAsync(s->qs_buf + o_pv, in.data(), in.size(), hipMemcpyHostToDevice, s->stream));
    const uint64_t rows = s->qs_hi - s->qs_lo;
    if (rows > 0) {
        uint32_t kw_min = QS_SLOTS;
        for (size_t t = 0; t < n_tiles; ++t) kw_min = std::min(kw_min, tiles[4 * t + 3]);
        const uint64_t cpw = (uint64_t)(QS_THREADS / kw_min);
        uint64_t nby = 1;
        CK(rows_grid(rows, n_tiles, QS_UNR * cpw, "bpm_quantile_histogram", &nby));
        hipLaunchKernelGGL(qs_histogram_kernel, dim3((unsigned)n_tiles, (unsigned)nby), dim3(QS_THREADS), 0, s->stream, (const double*)s->hist,
                           s->ld, s->qs_lo, s->qs_hi, reinterpret_cast<const uint4*>(s->qs_buf + o_tiles),
                           reinterpret_cast<const uint32_t*>(s->qs_buf + o_pk), reinterpret_cast<const uint64_t*>(s->qs_buf + o_pv), bits,
                           reinterpret_cast<unsigned long long*>(s->qs_buf), reinterpret_cast<unsigned long long*>(s->qs_buf + o_nan));
        HIPCK(hipGetLastError());
    }
    std::vector<uint64_t> out(np * 257);
    HIPCK(hipMemcpyAsync(out.data(), s->qs_buf, o_pv, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    std::memcpy(hist, out.data(), np * 256 * 8);
    if (n_nan)
        for (size_t j = 0; j < np; ++j) n_nan[j] = (int64_t)out[np * 256 + j];
    return 0;
}

// ---- posterior covariance (covariance.h; bipymc_amd/covariance.py chooses the centre, merges the ranks and finishes cov / corr) ---------
// Over the window of super-chain rows >= n_burn (bpm_reduce_moments' selection): sum[k] = sum (x_k - center_k), cross[i * dim + j] = sum
// (x_i - center_i)(x_j - center_j) (full and exactly symmetric), count = this rank's rows.  Keeps no state; every buffer is temporary.
namespace {
template <int T>
void cov_launch_diag(dim3 grid, hipStream_t st, const double* H, uint32_t ld, uint32_t dim, uint64_t r_lo, uint64_t r_hi, const double* c,
                     uint32_t n_blk, double* part, double* part1) {
    hipLaunchKernelGGL((cov_partial_kernel<T, true>), grid, dim3(64), 0, st, H, ld, dim, r_lo, r_hi, c, n_blk, part, part1);
}
}  // namespace
constexpr uint32_t COV_DIM_LIMIT = 16384;      // 256 blocks of COV_BLK tiles: 32640 block pairs, below the grid's 65535

extern "C" int bpm_reduce_cov(bpm_handle_t s, int64_t n_burn, const double* center, double* sum, double* cross, int64_t* count) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!center || !sum || !cross || !count) return fail("bpm_reduce_cov: null argument");
    CK(require_resident_history(s, "bpm_reduce_cov"));
    const uint32_t dim = s->dim;
    if (dim > COV_DIM_LIMIT)
        return fail("bpm_reduce_cov: dim = " + std::to_string(dim) + " is beyond the supported limit of " + std::to_string(COV_DIM_LIMIT) +
                    " coordinates");
    uint64_t r_lo = 0, r_hi = 0;
    CK(super_chain_window(s, n_burn, &r_lo, &r_hi));
    const uint64_t rows = r_hi - r_lo;
    *count = (int64_t)rows;
    if (rows == 0) {
        HIPCK(hipStreamSynchronize(s->stream));
        std::fill(sum, sum + dim, 0.0);
        std::fill(cross, cross + (size_t)dim * dim, 0.0);
        return 0;
    }
    const uint32_t n_tiles = (dim + 15u) / 16u;
    const uint32_t T = n_tiles <= (uint32_t)COV_MAX_T ? n_tiles : (uint32_t)COV_BLK;
    const uint32_t n_blk = (n_tiles + T - 1u) / T;
    const uint32_t n_off = n_blk * (n_blk - 1u) / 2u, n_slots = n_blk + n_off;
    // one wavefront per workgroup: one per SIMD where the accumulators take more than half of the register file, two otherwise
    const uint64_t n_grp = (rows + 3u) / 4u;
    const uint32_t want = T > (uint32_t)COV_BLK ? 1024u : 2048u;
    const uint32_t nbx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want / std::max(n_blk, std::max(n_off, 1u)),
                                                                            (n_grp + COV_UNR - 1) / COV_UNR));
    const size_t part_n = (size_t)n_slots * nbx * T * T * 256, part1_n = (size_t)n_blk * nbx * T * 64, cross_n = (size_t)dim * dim;
    const size_t need = (part_n + part1_n + cross_n + 2 * (size_t)dim) * sizeof(double);
    size_t mem_free = 0, mem_total = 0;
    HIPCK(hipMemGetInfo(&mem_free, &mem_total));
    if (need > mem_free)
        return fail("bpm_reduce_cov: dim = " + std::to_string(dim) + " needs " + std::to_string(need >> 20) +
                    " MiB of device memory for the dim x dim result and its partial sums; " + std::to_string(mem_free >> 20) + " MiB are free");
    DevTemp<double> d_center, d_part, d_part1, d_cross, d_sum;
    CK(d_center.alloc(dim));
    CK(d_part.alloc(part_n));
    CK(d_part1.alloc(part1_n));
    CK(d_cross.alloc(cross_n));
    CK(d_sum.alloc(dim));
    HIPCK(hipMemcpyAsync(d_center.p, center, dim * sizeof(double), hipMemcpyHostToDevice, s->stream));
    const dim3 gd(nbx, n_blk);
    const double* H = s->hist;
    switch (T) {
        case 1: cov_launch_diag<1>(gd, s->stream, H, s->ld, dim, r_lo, r_hi, d_center.p, n_blk, d_part.p, d_part1.p); break;
        case 2: cov_launch_diag<2>(gd, s->stream, H, s->ld, dim, r_lo, r_hi, d_center.p, n_blk, d_part.p, d_part1.p); break;
        case 3: cov_launch_diag<3>(gd, s->stream, H, s->ld, dim, r_lo, r_hi, d_center.p, n_blk, d_part.p, d_part1.p); break;
        case 4: cov_launch_diag<4>(gd, s->stream, H, s->ld, dim, r_lo, r_hi, d_center.p, n_blk, d_part.p, d_part1.p); break;
        case 5: cov_launch_diag<5>(gd, s->stream, H, s->ld, dim, r_lo, r_hi, d_center.p, n_blk, d_part.p, d_part1.p); break;
        case 6: cov_launch_diag<6>(gd, s->stream, H, s->ld, dim, r_lo, r_hi, d_center.p, n_blk, d_part.p, d_part1.p); break;
        default: cov_launch_diag<7>(gd, s->stream, H, s->ld, dim, r_lo, r_hi, d_center.p, n_blk, d_part.p, d_part1.p); break;
    }
    if (n_off > 0)
        hipLaunchKernelGGL((cov_partial_kernel<COV_BLK, false>), dim3(nbx, n_off), dim3(64), 0, s->stream, H, s->ld, dim, r_lo, r_hi,
                           (const double*)d_center.p, n_blk, d_part.p, d_part1.p);
    hipLaunchKernelGGL(cov_final_kernel, dim3(T * T, n_slots), dim3(COV_FIN_THREADS), 0, s->stream, (const double*)d_part.p, nbx, T, n_blk, dim,
                       d_cross.p);
    hipLaunchKernelGGL(cov_sum_final_kernel, dim3(n_tiles), dim3(256), 0, s->stream, (const double*)d_part1.p, nbx, T, dim, d_sum.p);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(cross, d_cross.p, cross_n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(sum, d_sum.p, dim * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

// ---- posterior histograms (histograms.h; bipymc_amd/histograms.py applies NumPy's range rules, builds the edges and merges the ranks) ----
// The counts of the reference's corner plot (corner.corner(samples), mc_plot/mc_plot.py:16-29), taken where the history lives.
constexpr uint32_t HS_LDS_TILE = 40u * 1024u;       // edges + one copy of the counts of a marginal tile
constexpr uint32_t HS_LDS_TOTAL = 48u * 1024u;      // ... with the extra copies
constexpr uint32_t HS_LDS_PAIRS = 32u * 1024u;      // the 2-D counts of a pair tile
constexpr uint32_t HS_TILE_PAIRS = 64;              // pairs per tile at most (128 distinct slots: two rows side by side in phase 1)

// Fixes the window of super-chain rows >= n_burn (bpm_reduce_moments' selection) for the bpm_hist_marginals / bpm_hist_pairs calls that
// follow and returns, per coordinate over this rank's rows: lo / hi = min / max of the values that are not NaN (+inf / -inf where there is
// none), n_nan and n_inf = how many are NaN / infinite; count = the rows.
extern "C" int bpm_hist_range(bpm_handle_t s, int64_t n_burn, double* lo, double* hi, int64_t* n_nan, int64_t* n_inf, int64_t* count) {
    CK(check_handle(s));
    CK(set_device(s));
    s->hs_seen.valid = false;
    if (!lo || !hi || !n_nan || !n_inf || !count) return fail("bpm_hist_range: null argument");
    CK(require_resident_history(s, "bpm_hist_range"));
    CK(super_chain_window(s, n_burn, &s->hs_lo, &s->hs_hi));
    s->hs_seen.take(s);
    const uint64_t rows = s->hs_hi - s->hs_lo;
    *count = (int64_t)rows;
    const uint32_t ld = s->ld, dim = s->dim;
    const uint64_t k_pinf = 0xFFF0000000000000ull, k_ninf = 0x000FFFFFFFFFFFFFull;      // qs_key(+inf), qs_key(-inf)
    std::vector<uint64_t> out((size_t)4 * ld, 0);
    std::fill(out.begin(), out.begin() + ld, k_pinf);
    std::fill(out.begin() + ld, out.begin() + 2 * (size_t)ld, k_ninf);
    if (rows > 0) {
        DevTemp<unsigned char> b;
        CK(b.alloc(out.size() * 8, "bpm_hist_range", "the per-coordinate results"));
        HIPCK(hipMemcpyAsync(b.p, out.data(), out.size() * 8, hipMemcpyHostToDevice, s->stream));
        const uint32_t kw = std::min<uint32_t>(ld, HS_THREADS), n_tiles = (ld + kw - 1) / kw;
        uint64_t nby = 1;
        CK(rows_grid(rows, n_tiles, (uint64_t)(HS_THREADS / kw) * HS_UNR, "bpm_hist_range", &nby));
        hipLaunchKernelGGL(hs_range_kernel, dim3(n_tiles, (unsigned)nby), dim3(HS_THREADS), 0, s->stream, (const double*)s->hist, ld, s->hs_lo,
                           s->hs_hi, kw, reinterpret_cast<unsigned long long*>(b.p));
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(out.data(), b.p, out.size() * 8, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
    }
    auto unkey = [](uint64_t k) {
        const uint64_t bits = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
        double x;
        std::memcpy(&x, &bits, 8);
        return x;
    };
    for (uint32_t k = 0; k < dim; ++k) {
        lo[k] = unkey(out[k]);
        hi[k] = unkey(out[(size_t)ld + k]);
        n_nan[k] = (int64_t)out[(size_t)2 * ld + k];
        n_inf[k] = (int64_t)out[(size_t)3 * ld + k];
    }
    return 0;
}

// counts[j * bins + i] = rows of the window of the last bpm_hist_range whose coordinate dims[j] lies in bin i of edges[j * (bins + 1) ...]
// (e[i] <= x < e[i + 1], the last bin closed; NaN and values outside are counted nowhere): np.histogram's counts for these edges.
extern "C" int bpm_hist_marginals(bpm_handle_t s, int32_t n_dims, const int32_t* dims, int32_t bins, const double* edges, int64_t* counts) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!dims || !edges || !counts) return fail("bpm_hist_marginals: null argument");
    CK(s->hs_seen.check(s, "bpm_hist_marginals", "bpm_hist_range"));
    if (bins < 1 || bins > HS_MAX_BINS)
        return fail("bpm_hist_marginals: bins = " + std::to_string(bins) + " is outside the supported 1 ... " + std::to_string(HS_MAX_BINS));
    if (n_dims < 1 || (uint32_t)n_dims > s->dim) return fail("bpm_hist_marginals: n_dims must be 1 ... dim");
    const uint32_t m = (uint32_t)n_dims, nb = (uint32_t)bins;
    CK(check_dims_edges(s, "bpm_hist_marginals", m, dims, nb, edges));
    const size_t n_counts = (size_t)m * nb, n_edges = (size_t)m * (nb + 1);
    std::fill(counts, counts + n_counts, (int64_t)0);
    const uint64_t rows = s->hs_hi - s->hs_lo;
    if (rows == 0) return 0;
    // [counts u64 | edges f64 | dims u32]
    const size_t o_e = n_counts * 8, o_d = o_e + n_edges * 8, need = o_d + (size_t)m * 4;
    DevTemp<unsigned char> b;
    CK(b.alloc(need, "bpm_hist_marginals", "the counts and edges"));
    std::vector<unsigned char> in(need - o_e);
    std::memcpy(in.data(), edges, n_edges * 8);
    stage_dims(in.data() + (o_d - o_e), dims, m);
    HIPCK(hipMemsetAsync(b.p, 0, o_e, s->stream));
    HIPCK(hipMemcpyAsync(b.p + o_e, in.data(), in.size(), hipMemcpyHostToDevice, s->stream));
    // a tile: kw slots whose edges and counts fit HS_LDS_TILE; rep copies of the counts while they fit HS_LDS_TOTAL
    const uint32_t slot_bytes = nb * 4 + (nb + 1) * 8;
    const uint32_t kw = std::max(1u, std::min({m, (uint32_t)HS_THREADS, HS_LDS_TILE / slot_bytes}));
    const uint32_t n_tiles = (m + kw - 1) / kw, cpw = HS_THREADS / kw;
    const uint32_t rep = std::max(1u, std::min({8u, cpw, (HS_LDS_TOTAL - kw * (nb + 1) * 8) / (kw * nb * 4)}));
    const uint32_t lds = kw * (nb + 1) * 8 + rep * kw * nb * 4;
    uint64_t nby = 1;
    CK(rows_grid(rows, n_tiles, (uint64_t)cpw * HS_UNR, "bpm_hist_marginals", &nby));
    hipLaunchKernelGGL(hs_marginal_kernel, dim3(n_tiles, (unsigned)nby), dim3(HS_THREADS), lds, s->stream, (const double*)s->hist, s->ld,
                       s->hs_lo, s->hs_hi, reinterpret_cast<const uint32_t*>(b.p + o_d), m, nb, reinterpret_cast<const double*>(b.p + o_e), kw,
                       rep, reinterpret_cast<unsigned long long*>(b.p));
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(counts, b.p, o_e, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

// counts2d[(p * bins2d + i) * bins2d + j] = rows of that window whose coordinate dims[pair_a[p]] lies in bin i of edges2d[pair_a[p]] and
// whose coordinate dims[pair_b[p]] lies in bin j of edges2d[pair_b[p]] (pair_a / pair_b index dims; the binning rule of the marginals):
// np.histogram2d's counts for these edges.
extern "C" int bpm_hist_pairs(bpm_handle_t s, int32_t n_dims, const int32_t* dims, int32_t bins2d, const double* edges2d, int64_t n_pairs,
                              const int32_t* pair_a, const int32_t* pair_b, int64_t* counts2d) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!dims || !edges2d || !pair_a || !pair_b || !counts2d) return fail("bpm_hist_pairs: null argument");
    CK(s->hs_seen.check(s, "bpm_hist_pairs", "bpm_hist_range"));
    if (bins2d < 1 || bins2d > HS_MAX_BINS2D)
        return fail("bpm_hist_pairs: bins2d = " + std::to_string(bins2d) + " is outside the supported 1 ... " + std::to_string(HS_MAX_BINS2D));
    if (n_dims < 1 || (uint32_t)n_dims > s->dim) return fail("bpm_hist_pairs: n_dims must be 1 ... dim");
    if (n_pairs < 1 || n_pairs > ((int64_t)1 << 24))
        return fail("bpm_hist_pairs: n_pairs = " + std::to_string(n_pairs) + " is outside the supported 1 ... 16777216");
    const uint32_t m = (uint32_t)n_dims, nb = (uint32_t)bins2d, cells = nb * nb;
    const size_t P = (size_t)n_pairs;
    CK(check_dims_edges(s, "bpm_hist_pairs", m, dims, nb, edges2d));
    for (size_t p = 0; p < P; ++p)
        if (pair_a[p] < 0 || pair_a[p] >= n_dims || pair_b[p] < 0 || pair_b[p] >= n_dims)
            return fail("bpm_hist_pairs: a pair names a coordinate that is not in dims");
    const size_t n_counts = P * cells, n_edges = (size_t)m * (nb + 1);
    const uint64_t rows = s->hs_hi - s->hs_lo;
    // tiles of pairs in the order given: equal shares of at most tp_max pairs; each tile's distinct slots in order of first use
    const uint32_t tp_max = std::max(1u, std::min(HS_TILE_PAIRS, HS_LDS_PAIRS / (cells * 4)));
    const size_t n_tiles = (P + tp_max - 1) / tp_max;
    const size_t tp = (P + n_tiles - 1) / n_tiles;
    std::vector<uint32_t> tiles, uslot, pl(2 * P);
    uint32_t nu_max = 1, np_max = 1;
    std::vector<int32_t> where(m, -1);
    for (size_t p0 = 0; p0 < P; p0 += tp) {
        const size_t np = std::min(tp, P - p0);
        const uint32_t u0 = (uint32_t)uslot.size();
        for (size_t p = p0; p < p0 + np; ++p)
            for (int side = 0; side < 2; ++side) {
                const int32_t sl = side ? pair_b[p] : pair_a[p];
                if (where[sl] < (int32_t)u0) {
                    where[sl] = (int32_t)uslot.size();
                    uslot.push_back((uint32_t)sl);
                }
                pl[2 * p + side] = (uint32_t)where[sl] - u0;
            }
        const uint32_t nu = (uint32_t)uslot.size() - u0;
        tiles.insert(tiles.end(), {(uint32_t)p0, (uint32_t)np, u0, nu});
        nu_max = std::max(nu_max, nu);
        np_max = std::max(np_max, (uint32_t)np);
    }
    // [counts u64 | edges f64 | tiles 16 B each | pl 8 B each | uslot u32 | dims u32]
    const size_t o_e = n_counts * 8, o_t = o_e + n_edges * 8, o_pl = o_t + n_tiles * 16, o_u = o_pl + P * 8, o_d = o_u + uslot.size() * 4,
                 need = o_d + (size_t)m * 4;
    DevTemp<unsigned char> b;
    CK(b.alloc(need, "bpm_hist_pairs",
               std::to_string(n_pairs) + " pairs of " + std::to_string(bins2d) + " x " + std::to_string(bins2d) + " 64-bit counts"));
    std::fill(counts2d, counts2d + n_counts, (int64_t)0);
    if (rows == 0) return 0;
    std::vector<unsigned char> in(need - o_e);
    std::memcpy(in.data(), edges2d, n_edges * 8);
    std::memcpy(in.data() + (o_t - o_e), tiles.data(), n_tiles * 16);
    std::memcpy(in.data() + (o_pl - o_e), pl.data(), P * 8);
    std::memcpy(in.data() + (o_u - o_e), uslot.data(), uslot.size() * 4);
    stage_dims(in.data() + (o_d - o_e), dims, m);
    HIPCK(hipMemsetAsync(b.p, 0, o_e, s->stream));
    HIPCK(hipMemcpyAsync(b.p + o_e, in.data(), in.size(), hipMemcpyHostToDevice, s->stream));
    const uint32_t lds = nu_max * (nb + 1) * 8 + np_max * cells * 4 + HS_THREADS * HS_UNR;
    uint64_t nby = 1;
    CK(rows_grid(rows, n_tiles, (uint64_t)(HS_THREADS / nu_max) * HS_UNR, "bpm_hist_pairs", &nby));
    hipLaunchKernelGGL(hs_pair_kernel, dim3((unsigned)n_tiles, (unsigned)nby), dim3(HS_THREADS), lds, s->stream, (const double*)s->hist, s->ld,
                       s->hs_lo, s->hs_hi, reinterpret_cast<const uint4*>(b.p + o_t), reinterpret_cast<const uint32_t*>(b.p + o_u),
                       reinterpret_cast<const uint2*>(b.p + o_pl), reinterpret_cast<const uint32_t*>(b.p + o_d), nb,
                       reinterpret_cast<const double*>(b.p + o_e), nu_max, np_max, reinterpret_cast<unsigned long long*>(b.p));
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(counts2d, b.p, o_e, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

// ---- per-generation trace summaries (traces.h; bipymc_amd/traces.py merges the ranks and finishes mean and sd) --------------------------
// What the reference's trace plots show (plot_mcmc_indep_chains / plot_mcmc_chain, mc_plot/mc_plot.py:52-102: every chain against the
// generation, np.mean and np.std per generation), taken where the history lives instead of from param_est(n_burn=0)'s copy of it.

// workgroups per bin along its rows.  Many short bins need none beyond the first; few long bins (every large) are cut so that the grid
// still fills the chip: rows_grid's rule with the (tile, bin) pairs in the place of its tiles -- about 2048 workgroups in all, each at
// least 4 sweeps of `rows_per_sweep` rows, none with 2^31 rows or more
static int trace_parts(uint64_t rows_per_bin, uint64_t tiles_x_bins, uint64_t rows_per_sweep, uint64_t* parts) {
    return rows_grid(rows_per_bin, tiles_x_bins, rows_per_sweep, "bpm_trace_bins", parts);
}

// Bins t = 0 .. T - 1, T = ceil((g_hi - g_lo) / every), of the generations [g_lo + t every, min(g_lo + (t + 1) every, g_hi)) over this
// rank's chains.  bin_counts: [2][T][dim] = how many values are finite | NaN; bin_sums: [5][T][dim] = shift c | sum (x - c) | sum (x - c)^2
// over the finite values | min | max over the values that are not NaN (+inf / -inf where there is none).  ll_counts: [4][T] = finite | NaN |
// +inf | -inf; ll_sums: [5][T] likewise for the ln-likes.  best_ll / best_row / best_x: the largest ln-like of the window that is not NaN,
// the smallest local row g * n_local + i that carries it and its dim coordinates (NaN, -1, NaN where every ln-like is NaN).
extern "C" int bpm_trace_bins(bpm_handle_t s, int64_t g_lo, int64_t g_hi, int64_t every, int64_t* bin_counts, double* bin_sums, int64_t* ll_counts,
                              double* ll_sums, double* best_ll, int64_t* best_row, double* best_x) {
    CK(check_handle(s));
    CK(set_device(s));
    s->tr_seen.valid = false;
    if (!bin_counts || !bin_sums || !ll_counts || !ll_sums || !best_ll || !best_row || !best_x) return fail("bpm_trace_bins: null argument");
    CK(require_resident_history(s, "bpm_trace_bins"));
    if (g_lo < 0 || g_hi < g_lo || g_hi > s->hist_rows) return fail("bpm_trace_bins: generation range out of bounds");
    if (every < 1) return fail("bpm_trace_bins: every must be >= 1 (got " + std::to_string((long long)every) + ")");
    CK(normalize_history(s, g_lo, g_hi));
    s->tr_g0 = g_lo; s->tr_g1 = g_hi; s->tr_every = every;
    s->tr_seen.take(s);
    const uint32_t ld = s->ld, dim = s->dim;
    *best_ll = std::nan("");
    *best_row = -1;
    std::fill(best_x, best_x + dim, std::nan(""));
    const uint64_t span = (uint64_t)(g_hi - g_lo);
    if (span == 0) return 0;
    const uint64_t ev = std::min<uint64_t>((uint64_t)every, span);      // (a bin wider than the window is the window)
    const uint64_t T = (span + ev - 1) / ev, rows_per_bin = ev * s->n_local;
    const uint32_t kw = std::min<uint32_t>(ld, TR_THREADS), n_tiles = (ld + kw - 1) / kw, cpw = TR_THREADS / kw;
    if (T * n_tiles >= (1ull << 31)) return fail("bpm_trace_bins: too many bins");
    uint64_t pb = 1, pl = 1;
    CK(trace_parts(rows_per_bin, T * n_tiles, (uint64_t)cpw * TR_UNR, &pb));
    CK(trace_parts(rows_per_bin, T, (uint64_t)TR_THREADS * TR_UNR, &pl));
    // [bins: part records | folded records][ln-likes: part records | folded records]; with one part the part records are the folded ones
    const uint64_t nb_out = T * ld, nb_rec = nb_out * pb, nl_out = T, nl_rec = T * pl;
    const size_t o_bf = (size_t)TR_F_BINS * nb_rec, o_lp = o_bf + (pb > 1 ? (size_t)TR_F_BINS * nb_out : 0);
    const size_t o_lf = o_lp + (size_t)TR_F_LL * nl_rec, need = o_lf + (pl > 1 ? (size_t)TR_F_LL * nl_out : 0);
    DevTemp<double> b;
    CK(b.alloc(need, "bpm_trace_bins", "the per-bin records of " + std::to_string((unsigned long long)T) + " bins"));
    double* bins_rec = b.p;
    double* ll_rec = b.p + o_lp;
    hipLaunchKernelGGL(tr_bins_kernel, dim3((unsigned)(T * n_tiles), (unsigned)pb), dim3(TR_THREADS), 0, s->stream, (const double*)s->hist, ld,
                       s->n_local, (uint64_t)g_lo, (uint64_t)g_hi, ev, kw, n_tiles, bins_rec, nb_rec);
    hipLaunchKernelGGL(tr_ll_kernel, dim3((unsigned)T, (unsigned)pl), dim3(TR_THREADS), 0, s->stream, (const double*)s->llhist, s->n_local,
                       (uint64_t)g_lo, (uint64_t)g_hi, ev, ll_rec, nl_rec);
    if (pb > 1) {
        hipLaunchKernelGGL(tr_fold_kernel, dim3((unsigned)((nb_out + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, s->stream,
                           (const double*)bins_rec, (uint32_t)pb, ld, nb_out, (uint32_t)TR_F_BINS, b.p + o_bf);
        bins_rec = b.p + o_bf;
    }
    if (pl > 1) {
        hipLaunchKernelGGL(tr_fold_kernel, dim3((unsigned)((nl_out + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, s->stream,
                           (const double*)ll_rec, (uint32_t)pl, 1u, nl_out, (uint32_t)TR_F_LL, b.p + o_lf);
        ll_rec = b.p + o_lf;
    }
    HIPCK(hipGetLastError());
    std::vector<double> hb((size_t)TR_F_BINS * nb_out), hl((size_t)TR_F_LL * nl_out);
    HIPCK(hipMemcpyAsync(hb.data(), bins_rec, hb.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(hl.data(), ll_rec, hl.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    auto word = [](const std::vector<double>& h, size_t i) {
        int64_t w;
        std::memcpy(&w, &h[i], 8);
        return w;
    };
    const int count_f[2] = {TR_N, TR_NAN}, sum_f[5] = {TR_C, TR_S1, TR_S2, TR_MIN, TR_MAX}, ll_count_f[4] = {TR_N, TR_NAN, TR_PINF, TR_NINF};
    const size_t td = (size_t)T * dim;
    for (uint64_t t = 0; t < T; ++t)
        for (uint32_t k = 0; k < dim; ++k) {
            const size_t src = (size_t)t * ld + k, dst = (size_t)t * dim + k;
            for (int f = 0; f < 2; ++f) bin_counts[f * td + dst] = word(hb, (size_t)count_f[f] * nb_out + src);
            for (int f = 0; f < 5; ++f) bin_sums[f * td + dst] = hb[(size_t)sum_f[f] * nb_out + src];
        }
    uint64_t bkey = 0, brow = TR_NO_ROW;
    for (uint64_t t = 0; t < T; ++t) {
        for (int f = 0; f < 4; ++f) ll_counts[f * T + t] = word(hl, (size_t)ll_count_f[f] * nl_out + t);
        for (int f = 0; f < 5; ++f) ll_sums[f * T + t] = hl[(size_t)sum_f[f] * nl_out + t];
        const uint64_t kb = (uint64_t)word(hl, (size_t)TR_BKEY * nl_out + t), rb = (uint64_t)word(hl, (size_t)TR_BROW * nl_out + t);
        if (kb > bkey || (kb == bkey && rb < brow)) { bkey = kb; brow = rb; }      // bins in order: the larger key, then the smaller row
    }
    if (brow != TR_NO_ROW) {
        if (brow >= (uint64_t)s->hist_rows * s->n_local) return fail("bpm_trace_bins: internal error (arg-max row out of range)");
        HIPCK(hipMemcpyAsync(best_ll, s->llhist + brow, sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipMemcpyAsync(best_x, s->hist + brow * ld, dim * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        *best_row = (int64_t)brow;
    }
    return 0;
}

// The local chains local_ids[0 .. n) at the first generation of every bin of the last bpm_trace_bins, T bins:
// out_x[(t * n + j) * dim + k] and out_ll[t * n + j] = chain local_ids[j] at generation g_lo + t * every.
extern "C" int bpm_trace_chains(bpm_handle_t s, int32_t n, const int32_t* local_ids, double* out_x, double* out_ll) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!local_ids || !out_x || !out_ll) return fail("bpm_trace_chains: null argument");
    CK(s->tr_seen.check(s, "bpm_trace_chains", "bpm_trace_bins"));
    if (n < 1 || (uint32_t)n > s->n_local) return fail("bpm_trace_chains: n must be 1 ... n_local");
    for (int32_t j = 0; j < n; ++j)
        if (local_ids[j] < 0 || (uint32_t)local_ids[j] >= s->n_local)
            return fail("bpm_trace_chains: local chain " + std::to_string(local_ids[j]) + " is outside [0, " + std::to_string(s->n_local) + ")");
    const uint64_t span = (uint64_t)(s->tr_g1 - s->tr_g0);
    if (span == 0) return 0;
    const uint64_t ev = std::min<uint64_t>((uint64_t)s->tr_every, span), T = (span + ev - 1) / ev;
    const uint64_t n_x = T * (uint64_t)n * s->dim, n_ll = T * (uint64_t)n, n_el = n_x + n_ll;
    if ((n_el + TR_THREADS - 1) / TR_THREADS >= (1ull << 31)) return fail("bpm_trace_chains: too many bins x chains");
    // [out_x | out_ll | ids u32]
    DevTemp<double> b;
    CK(b.alloc((size_t)n_el + ((size_t)n + 1) / 2, "bpm_trace_chains", "the gathered chains"));
    uint32_t* d_ids = reinterpret_cast<uint32_t*>(b.p + n_el);
    std::vector<unsigned char> ids((size_t)n * 4);
    stage_dims(ids.data(), local_ids, (size_t)n);
    HIPCK(hipMemcpyAsync(d_ids, ids.data(), ids.size(), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(tr_gather_kernel, dim3((unsigned)((n_el + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, s->stream, (const double*)s->hist,
                       (const double*)s->llhist, s->ld, s->dim, s->n_local, (uint64_t)s->tr_g0, ev, T, (uint32_t)n, (const uint32_t*)d_ids, b.p,
                       b.p + n_x);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(out_x, b.p, (size_t)n_x * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(out_ll, b.p + n_x, (size_t)n_ll * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int bpm_synchronize(bpm_handle_t s) {
    CK(check_handle(s));
    CK(set_device(s));
    CK(wait_stream(s->stream));
    return push_check_error(s);
}

// ---- host-callback ln_like_fn (samplers.py:36-43): one half generation = proposals out, ln-likes in ------------------------------------------------
// Round 5: ONE core in three transports.  The proposal kernel writes the half generation's proposals (work-item order) into prop_buf and the
// snooker corrections into aux_buf[0 .. n_local); the ln-likes arrive in aux_buf[n_local ..) -- from pinned host memory chunk by chunk while the
// caller evaluates (bpm_propose_begin / _chunk, bpm_commit_chunk / _end), through the caller-owned buffers of rounds 1-4 (bpm_propose / bpm_commit:
// the same calls with one chunk and a compaction copy), or from DEVICE memory the caller's own framework computed them in (bpm_propose_device /
// bpm_commit_device: no PCIe).  Then the commit kernel: Metropolis (samplers.py:328-336), append (chain.py:51-54), CR statistics.
static int propose_launch(bpm_sampler* s, const char* who, bool clear_ids = true) {
    if (!s->run_open) return fail(std::string(who) + ": call bpm_begin_run first");
    if (s->cfg.target_id != BPM_TARGET_HOST_CALLBACK) return fail(std::string(who) + ": sampler has a device target; use bpm_step");
    if (s->proposed) return fail(std::string(who) + ": previous proposals not committed");
    if (s->phase == 0) CK(prepare_generation(s, 1));
    const PhaseArgs& a = s->cur_args[s->phase];
    // (only entries the proposal kernel does not write -- work items beyond n_items, which nobody reads: kept for the host transports as rounds 1-4 had it)
    if (clear_ids) HIPCK(hipMemsetAsync(s->ids_buf, 0xFF, s->n_local * sizeof(int32_t), s->stream));
    if (a.n_items > 0) g_propose[s->cfg.algo == BPM_ALGO_DREAM ? 1 : 0][s->shape.idx](a, s->stream);
    HIPCK(hipGetLastError());
    return 0;
}
// the commit kernel + the bookkeeping of the half generation (the ln-likes of every active work item are in aux_buf[n_local ..) on the stream by now)
static int commit_finish(bpm_sampler* s, int64_t n_active, bool sync = true) {
    const PhaseArgs& a = s->cur_args[s->phase];
    if (a.n_items > 0) g_commit[s->cfg.algo == BPM_ALGO_DREAM ? 1 : 0][s->shape.idx](a, s->stream);
    HIPCK(hipGetLastError());
    if (s->cfg.algo == BPM_ALGO_DEMC_SYNC) {       // one propose/commit per generation: apply the banked updates
        HIPCK(hipMemcpyAsync(s->G + (uint64_t)s->rank * s->L.blk, s->x_next, (size_t)s->n_local * s->ld * sizeof(double),
                             hipMemcpyDeviceToDevice, s->stream));
        CK(allgather_state(s));
        HIPCK(hipStreamSynchronize(s->stream));
        s->proposed = false; s->prop_mode = 0;
        return finish_generation(s);       // (synchronous DE-MC: never DREAM, no outlier check)
    }
    CK(allgather_state(s));
    if (sync) HIPCK(hipStreamSynchronize(s->stream));
    s->proposed = false; s->prop_mode = 0;
    if (s->phase == 0) {
        s->phase = 1;
        s->phase_a_updates = n_active;
    } else {
        s->phase = 0;
        CK(finish_generation(s));
        if (s->outlier_due) { bpm_sampler* one[1] = {s}; CK(group_outlier_check(Group{one, 1, s->comm != nullptr})); }
    }
    return 0;
}
static inline uint32_t chunk_lo(uint32_t n_items, int32_t n_chunks, int32_t k) { return (uint32_t)(((uint64_t)n_items * (uint64_t)k) / (uint64_t)n_chunks); }

extern "C" int bpm_propose_begin(bpm_handle_t s, int32_t n_chunks) {
    CK(check_handle(s));
    CK(set_device(s));
    if (n_chunks < 1 || n_chunks > 256) return fail("bpm_propose_begin: 1 <= n_chunks <= 256");
    CK(propose_launch(s, "bpm_propose_begin"));
    const PhaseArgs& a = s->cur_args[s->phase];
    while ((int32_t)s->chunk_ev.size() < n_chunks) {
        hipEvent_t e = nullptr;
        HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        s->chunk_ev.push_back(e);
    }
    // the ids first (32 KB), then the proposals chunk by chunk, an event behind each: the DMA of chunk k + 1 runs while the caller evaluates chunk k
    HIPCK(hipMemcpyAsync(s->h_ids, s->ids_buf, s->n_local * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    for (int32_t k = 0; k < n_chunks; ++k) {
        const uint32_t w0 = chunk_lo(a.n_items, n_chunks, k), w1 = chunk_lo(a.n_items, n_chunks, k + 1);
        if (w1 > w0)
            HIPCK(hipMemcpyAsync(s->h_props + (size_t)w0 * s->ld, s->prop_buf + (size_t)w0 * s->ld, (size_t)(w1 - w0) * s->ld * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipEventRecord(s->chunk_ev[(size_t)k], s->stream));
    }
    s->prop_chunks = n_chunks; s->prop_mode = 1; s->prop_given = 0; s->prop_active = 0; s->prop_whole = false;
    s->prop_done.assign((size_t)n_chunks, 0);
    s->proposed = true;
    return 0;
}

extern "C" int bpm_propose_chunk(bpm_handle_t s, int32_t k, const double** rows, const int32_t** ids, int32_t* n_rows, int32_t* ld) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->proposed || s->prop_mode != 1) return fail("bpm_propose_chunk: call bpm_propose_begin first");
    if (k < 0 || k >= s->prop_chunks || !rows || !ids || !n_rows || !ld) return fail("bpm_propose_chunk: bad argument");
    const PhaseArgs& a = s->cur_args[s->phase];
    HIPCK(hipEventSynchronize(s->chunk_ev[(size_t)k]));
    const uint32_t w0 = chunk_lo(a.n_items, s->prop_chunks, k), w1 = chunk_lo(a.n_items, s->prop_chunks, k + 1);
    *rows = s->h_props + (size_t)w0 * s->ld;
    *ids = s->h_ids + w0;
    *n_rows = (int32_t)(w1 - w0);
    *ld = (int32_t)s->ld;
    return 0;
}

extern "C" int bpm_commit_chunk(bpm_handle_t s, int32_t k, const double* ll) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->proposed || s->prop_mode != 1) return fail("bpm_commit_chunk: call bpm_propose_begin first");
    if (k < 0 || k >= s->prop_chunks) return fail("bpm_commit_chunk: bad chunk");
    if (s->prop_done[(size_t)k]) return fail("bpm_commit_chunk: the values of piece " + std::to_string(k) + " were handed in already");
    const PhaseArgs& a = s->cur_args[s->phase];
    const uint32_t w0 = chunk_lo(a.n_items, s->prop_chunks, k), w1 = chunk_lo(a.n_items, s->prop_chunks, k + 1);
    if (w1 > w0) {
        if (!ll) return fail("bpm_commit_chunk: null ll");
        // (into pinned staging first: the caller's array may be gone before the copy runs)
        std::memcpy(s->h_ll + w0, ll, (size_t)(w1 - w0) * sizeof(double));
        for (uint32_t w = w0; w < w1; ++w) s->prop_active += s->h_ids[w] >= 0 ? 1 : 0;
        HIPCK(hipMemcpyAsync(s->aux_buf + s->n_local + w0, s->h_ll + w0, (size_t)(w1 - w0) * sizeof(double), hipMemcpyHostToDevice, s->stream));
    }
    s->prop_done[(size_t)k] = 1;
    s->prop_given += 1;
    return 0;
}

extern "C" int bpm_commit_end(bpm_handle_t s) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->proposed || s->prop_mode != 1) return fail("bpm_commit_end: nothing proposed with bpm_propose_begin");
    s->prop_whole = false;
    if (s->prop_given != s->prop_chunks) return fail("bpm_commit_end: " + std::to_string(s->prop_given) + " of " + std::to_string(s->prop_chunks) + " chunks were given their ln-likes (bpm_commit_chunk)");
    return commit_finish(s, s->prop_active);
}

// ---- the caller's likelihood as a kernel compiled from HIP source (user_likelihood.h): proposal kernel -> the caller's kernel -> commit kernel, all on the
// sampler's stream, no host code inside a generation.  samplers.py:36-43 evaluates ln_like_fn(theta, **ln_kwargs) row by row on the host; here `params` takes
// the place of ln_kwargs.
static constexpr size_t N_EMBEDDED = sizeof(bpm_embedded) / sizeof(bpm_embedded[0]);      // (embedded_src.h: the headers a run-time program may include)
static int user_eval_launch(bpm_sampler* s, const double* rows, const int32_t* ids, uint32_t n, double* out) {
    if (n == 0) return 0;
    int rpb = 0, ldp = 0;
    bpm::user_eval_tile(s->dim, rpb, ldp);
    const unsigned block = (unsigned)bpm::USER_EVAL_BLOCK, per = rpb > 0 ? (unsigned)rpb : block, grid = (n + per - 1u) / per;
    const unsigned lds = rpb > 0 ? (unsigned)rpb * (unsigned)ldp * (unsigned)sizeof(double) : 0u;
    HIPCK(ModuleLaunch<bpm::UserEvalKernel>::on(s->stream, s->like.fn, grid, block, lds, rows, ids, (int)n, (int)s->ld, (int)s->dim, s->like.params.p, out, rpb, ldp));
    return 0;
}
// The installed likelihood's kernel of its own on `n` rows (stride s->ld) -> out[n]: bpm_user_eval, or for the per-datum form a wavefront per
// (row, chunk of the data) and, with more than one chunk, the fold of the chunk sums (user_eval_data.h).  The chunking is a function of n_data alone;
// rows beyond the scratch's batch go in further launches, which changes no row's value.
static int user_ll_launch(bpm_sampler* s, const double* rows, const int32_t* ids, uint32_t n, double* out) {
    const UserLikelihood& u = s->like;
    if (u.n_data == 0) return user_eval_launch(s, rows, ids, n, out);
    for (uint32_t r0 = 0; r0 < n; r0 += u.batch_rows) {
        const uint32_t nb = std::min(u.batch_rows, n - r0);
        const uint64_t items = (uint64_t)nb * (uint64_t)u.n_chunks;      // (batch_rows keeps it below 2^31)
        const double* rb = rows + (size_t)r0 * s->ld;
        const int32_t* ib = ids ? ids + r0 : nullptr;
        const unsigned grid = (unsigned)((items + bpm::USER_DATA_WAVES - 1) / bpm::USER_DATA_WAVES);
        HIPCK(ModuleLaunch<bpm::UserEvalDataKernel>::on(s->stream, u.fn, grid, 64u * bpm::USER_DATA_WAVES, 0, rb, ib, (int)nb, (int)s->ld, (int)s->dim, u.params.p,
                                                        u.data.p, (int)u.n_data, (int)u.n_chunks, out + r0, u.part.p));
        if (u.n_chunks > 1)
            HIPCK(ModuleLaunch<bpm::UserFoldDataKernel>::on(s->stream, u.fold, (nb + 63u) / 64u, 64u, 0, rb, ib, (int)nb, (int)s->ld, (int)s->dim, u.params.p, u.part.p,
                                                            (int)u.n_data, (int)u.n_chunks, out + r0));
    }
    return 0;
}
// ln-like of the local chains' CURRENT states from the installed device likelihood (what bpm_set_loglike takes from the host)
static int user_refresh_ll(bpm_sampler* s) {
    const double* X = s->G + (uint64_t)s->rank * s->L.blk;
    if (s->like.fused.eval) {      // (the update kernel was compiled around the likelihood: the same Target::eval, the same bits)
        HIPCK(ModuleLaunch<bpm::UserEvalLlKernel>::on(s->stream, s->like.fused.eval, grid_for(s->n_local, s->shape.lpc), s->like.fused.block, 0, X, s->n_local, s->ld,
                                                      s->dim, s->like.params.p, s->ll));
    } else {
        CK(user_ll_launch(s, X, nullptr, s->n_local, s->ll));
    }
    if (last_row_is_state(s))
        HIPCK(hipMemcpyAsync(s->llhist + (size_t)(s->hist_rows - 1) * s->n_local, s->ll, s->n_local * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}
static int run_generations_user(bpm_sampler* s, int64_t n_gens) {
    // (a rank of a world exchanges through its RCCL communicator like the host transports do: allgather_state in commit_finish)
    if (s->world > 1 && !s->comm) return fail("bpm_step: a host-callback sampler of a world needs an RCCL communicator (create it with a unique id)");
    const int halves = s->cfg.algo == BPM_ALGO_DEMC_SYNC ? 1 : 2;
    for (int64_t g = 0; g < n_gens; ++g) {
        for (int h = 0; h < halves; ++h) {
            CK(propose_launch(s, "bpm_step", false));      // (the proposal kernel writes the id of EVERY work item below n_items, -1 for an idle one)
            const PhaseArgs& a = s->cur_args[s->phase];
            int64_t act = (int64_t)a.n_items;
            if (s->world > 1 && a.n_items > 0) {      // (a rank of a world: half of its work items sit in the other pool)
                HIPCK(hipMemcpyAsync(s->h_ids, s->ids_buf, s->n_local * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
                HIPCK(hipStreamSynchronize(s->stream));
                act = 0;
                for (uint32_t w = 0; w < a.n_items; ++w) act += s->h_ids[w] >= 0 ? 1 : 0;
            }
            CK(user_ll_launch(s, s->prop_buf, s->world > 1 ? s->ids_buf : nullptr, a.n_items, s->aux_buf + s->n_local));
            s->proposed = true; s->prop_mode = 3; s->prop_chunks = 0;
            CK(commit_finish(s, act, false));
        }
    }
    return 0;
}

extern "C" int bpm_check_device_likelihood(const char* hip_source, const char* arch, char* log, int64_t log_cap) {
    return check_source("bpm_check_device_likelihood", hip_source, arch, log, log_cap, [] { return 0; }, [&](const char* a, std::vector<char>& code) {
        return bpm::compile_user_likelihood(hip_source, a, bpm_embedded, N_EMBEDDED, code); });
}

#ifdef BPM_TEST_HOOKS
static constexpr bool USER_FUSED_HOOKS = true;
// Test hook: the update kernel's program around `hip_source` (compile_user_fused, as bpm_set_device_likelihood builds it for a sampler of this algorithm
// and shape) compiled with no device in the machine; the reason comes back in `log` like bpm_check_device_likelihood's
extern "C" int bpm_debug_check_user_fused(const char* hip_source, int32_t algo, int32_t lpc, int32_t dpl, int32_t np, int32_t dim, int32_t hot, const char* arch,
                                          char* log, int64_t log_cap) {
    std::string lowered[4];
    return check_source("bpm_debug_check_user_fused", hip_source, arch, log, log_cap, [] { return 0; }, [&](const char* a, std::vector<char>& code) {
        return bpm::compile_user_fused(hip_source, "v_user_check", a, bpm_embedded, N_EMBEDDED, algo == BPM_ALGO_DREAM ? ALGO_DREAM : ALGO_DEMC, lpc, dpl, np,
                                       (uint32_t)dim, USER_FUSED_HOOKS, hot, code, lowered); });
}
#else
static constexpr bool USER_FUSED_HOOKS = false;
#endif
// The faster form: the update kernel itself compiled around the likelihood, built whole into `f` on the sampler's device.  -> "" or why it cannot be
// used; whatever goes wrong leaves nothing behind (the module is owned from the moment it is loaded).
static std::string build_user_fused(bpm_sampler* s, const char* hip_source, const char* arch, UserLikelihood::Fused& f) {
    const int algo = s->cfg.algo == BPM_ALGO_DREAM ? ALGO_DREAM : ALGO_DEMC;
    const int np = s->cfg.algo != BPM_ALGO_DREAM ? 1 : (s->cfg.del_pairs == 3 ? 3 : 0);
    static std::atomic<int> module_no{0};
    const std::string ns = "v_user" + std::to_string(module_no.fetch_add(1));
    std::vector<char> code;
    std::string lowered[4];
    const std::string why = bpm::compile_user_fused(hip_source, ns, arch, bpm_embedded, N_EMBEDDED, algo, s->shape.lpc, s->shape.dpl, np, s->dim, USER_FUSED_HOOKS,
                                                    s->plan_on ? 1 : 2, code, lowered);
    if (!why.empty()) return why;
    if (f.mod.load(code) != hipSuccess) { (void)hipGetLastError(); return "hipModuleLoadData failed"; }
    f.fn = f.mod.function(lowered[0]);
    f.hot = f.mod.function(lowered[1]);
    f.eval = f.mod.function(lowered[2]);
    const hipFunction_t fs = f.mod.function("bpm_user_sizeof");
    if (!f.fn || !f.hot || !f.eval || !fs) return "the compiled module lacks " + lowered[0];
    if (!lowered[3].empty()) f.adapt = f.mod.function(lowered[3]);
    // the module's view of the argument block must be this library's
    DevTemp<unsigned int> d_out;
    unsigned int h_out[3] = {0u, 0u, 0u};
    if (d_out.alloc(3) != 0) return "out of device memory";
    const bool ran = ModuleLaunch<bpm::UserSizeofKernel>::on(s->stream, fs, 1, 1, 0, d_out.p) == hipSuccess &&
                     hipMemcpyAsync(h_out, d_out.p, sizeof(h_out), hipMemcpyDeviceToHost, s->stream) == hipSuccess && hipStreamSynchronize(s->stream) == hipSuccess;
    if (!ran || h_out[0] != (unsigned)sizeof(PhaseArgs) || h_out[1] != (unsigned)block_for(s->shape.lpc)) {
        (void)hipGetLastError();
        return "the module's argument block differs from the library's (" + std::to_string(h_out[0]) + " against " + std::to_string(sizeof(PhaseArgs)) + " bytes)";
    }
    f.block = h_out[1];
    f.block_adapt = h_out[2];
    if (f.adapt && h_out[2] != (unsigned)block_for_hot(s->shape.lpc, 3, s->shape.dpl)) f.adapt = nullptr;
    f.names[0] = lowered[0]; f.names[1] = lowered[1]; f.names[2] = lowered[3];
    static const bool dq_wanted = !(getenv("BPM_USER_FUSED") && atoi(getenv("BPM_USER_FUSED")) == 2);      // (2: fused, but launched on the stream -- A/B)
    f.dq = dq_wanted && s->dq && s->dq->kernel_by_name(lowered[0]) != nullptr && s->dq->kernel_by_name(lowered[1]) != nullptr &&
           (!f.adapt || s->dq->kernel_by_name(lowered[3]) != nullptr);
    return "";
}

// One way in for every form.  data == nullptr: the plain and the per-coordinate form (bpm_set_device_likelihood); else the per-datum form, its data
// (n_data, w) row-major copied into a buffer of the likelihood's own (bpm_set_device_likelihood_data).
static int install_user_likelihood(bpm_sampler* s, const std::string& who, const char* hip_source, const double* params, int32_t n_params, const double* data,
                                   int64_t n_data, int32_t w) {
    if (s->cfg.target_id != BPM_TARGET_HOST_CALLBACK) return fail(who + ": the sampler has a shipped device target (create it with BPM_TARGET_HOST_CALLBACK)");
    if (s->proposed) return fail(who + ": a half generation is open (bpm_propose ... without its commit)");
    if (!hip_source || n_params < 0 || (n_params > 0 && !params)) return fail(who + ": bad argument");
    const bool has_data = bpm::user_source_has_data(hip_source);
    if (!data && has_data) return fail(who + ": the source is in the per-datum form (BPM_LN_LIKE_DATA): give it its data with bpm_set_device_likelihood_data");
    if (data && !has_data) return fail(who + ": the source does not define BPM_LN_LIKE_DATA and BPM_LN_LIKE_DATA_W (the per-datum form: user_eval_data.h)");
    std::string arch;
    CK(device_arch(s->cfg.device, arch));
    const auto build = [&](UserLikelihood& next) {
        std::vector<char> code;
        const std::string why = bpm::compile_user_likelihood(hip_source, arch, bpm_embedded, N_EMBEDDED, code);
        if (!data) return load_kernels(who, why, code, next.mod, {{"bpm_user_eval", &next.fn}});
        hipFunction_t info = nullptr;
        CK(load_kernels(who, why, code, next.mod, {{"bpm_user_eval_data", &next.fn}, {"bpm_user_fold_data", &next.fold}, {"bpm_user_data_info", &info}}));
        // the program's view of K, w, the chunk and the workgroup must be this call's and this library's
        DevTemp<int> d_info;
        int h_info[4] = {0, 0, 0, 0};
        CK(d_info.alloc(4));
        HIPCK(ModuleLaunch<bpm::UserDataInfoKernel>::on(s->stream, info, 1, 1, 0, d_info.p));
        HIPCK(hipMemcpyAsync(h_info, d_info.p, sizeof(h_info), hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        const int K = h_info[0];
        if (K < 1 || K > 8 || h_info[2] != bpm::USER_DATA_CHUNK || h_info[3] != bpm::USER_DATA_WAVES) return fail(who + ": the compiled module's chunking differs from the library's");
        if (h_info[1] != w)
            return fail(who + ": the source was written for " + std::to_string(h_info[1]) + " values per datum (BPM_LN_LIKE_DATA_W), the data have " + std::to_string(w));
        next.n_data = (int32_t)n_data;
        next.n_chunks = (int32_t)((n_data + bpm::USER_DATA_CHUNK - 1) / bpm::USER_DATA_CHUNK);
        // rows of one launch: what the scratch bound admits, but no more than this sampler's own launches need -- its n_local chains, or 256 rows for a small
        // population, so that an evaluation of a few hundred given rows is still one launch.  bpm_eval_device_likelihood takes more rows in batches; no
        // value depends on the batching (tests/test_gpu_data_likelihood.py evaluates 257 rows, across a batch boundary, for that reason)
        const size_t row_bytes = (size_t)next.n_chunks * (size_t)K * sizeof(double);
        next.batch_rows = (uint32_t)std::min<size_t>(std::max<size_t>(bpm::USER_DATA_SCRATCH_BYTES / row_bytes, 1), std::max<size_t>(s->n_local, 256));
        next.batch_rows = (uint32_t)std::min<uint64_t>(next.batch_rows, (uint64_t)0x7fffffff / (uint64_t)next.n_chunks);
        CK(next.data.alloc((size_t)n_data * (size_t)w, who.c_str(), "the data"));
        HIPCK(hipMemcpyAsync(next.data.p, data, (size_t)n_data * (size_t)w * sizeof(double), hipMemcpyHostToDevice, s->stream));
        if (next.n_chunks > 1) CK(next.part.alloc((size_t)next.batch_rows * (size_t)next.n_chunks * (size_t)K, who.c_str(), "the chunk sums"));
        return 0;
    };
    // (install_function: the installed likelihood stays whole until nothing can fail any more; the old update kernel leaves with it)
    CK(install_function(s->stream, s->like, false, params, n_params, build, [&](UserLikelihood& old) { old.fused.drop(s->dq); }));
    CK(user_refresh_ll(s));     // (by the kernel of its own; again below by the update kernel's arithmetic once that one is built)
    if (data) { s->like.why = "the likelihood is summed over its data by kernels of its own (a wavefront per chunk of the data), not inside the update kernel"; return 0; }
    // the faster form.  Whatever goes wrong with it leaves the three-kernel form in place (bpm_get_device_likelihood_info says which is in use
    // and why).  BPM_USER_FUSED=0: not attempted (A/B, tests).
    const bool want_fused = !(getenv("BPM_USER_FUSED") && atoi(getenv("BPM_USER_FUSED")) == 0);      // (read at every call: a test switches it)
    UserLikelihood::Fused fused;
    s->like.why = !want_fused ? "BPM_USER_FUSED=0"
                  : s->shape.idx == SHAPE_WIDE ? "rows wider than 512 coordinates run on the looped kernel, which has no run-time form"
                                               : build_user_fused(s, hip_source, arch.c_str(), fused);
    if (!s->like.why.empty()) return 0;
    s->like.fused = std::move(fused);
    return user_refresh_ll(s);      // (again, now by the update kernel's own arithmetic: the per-coordinate form adds in the kernel's reduction order)
}

extern "C" int bpm_set_device_likelihood(bpm_handle_t s, const char* hip_source, const double* params, int32_t n_params) {
    CK(check_handle(s));
    CK(set_device(s));
    return install_user_likelihood(s, "bpm_set_device_likelihood", hip_source, params, n_params, nullptr, 0, 0);
}

// The per-datum form (user_eval_data.h): `data` (n_data, w) float64 row-major, copied to the device here and kept until the likelihood is replaced or the
// handle destroyed.  A single rank only: in a world the three-kernel path exchanges through RCCL.
extern "C" int bpm_set_device_likelihood_data(bpm_handle_t s, const char* hip_source, const double* params, int32_t n_params, const double* data, int64_t n_data,
                                              int32_t w) {
    CK(check_handle(s));
    CK(set_device(s));
    if (s->world > 1)
        return fail("bpm_set_device_likelihood_data: a likelihood with data runs on a single rank only (" + std::to_string(s->world) + " ranks here)");
    if (!data || n_data < 1 || n_data > (int64_t)0x7fffffff || w < 1 || w > bpm::USER_DATA_MAX_W)
        return fail("bpm_set_device_likelihood_data: data must be (n_data, w) with 1 <= n_data < 2^31 and 1 <= w <= " + std::to_string(bpm::USER_DATA_MAX_W));
    return install_user_likelihood(s, "bpm_set_device_likelihood_data", hip_source, params, n_params, data, n_data, w);
}

// the chunk of the data one wavefront sums in the per-datum form (user_eval_data.h: the order of the additions depends on it and on n_data alone)
extern "C" int bpm_data_likelihood_chunk(void) { return bpm::USER_DATA_CHUNK; }

// The installed device likelihood -- of any form -- on `n` given rows X (n, dim), by its kernel of its own (never the update kernel's arithmetic)
extern "C" int bpm_eval_device_likelihood(bpm_handle_t s, const double* X, int32_t n, double* out) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->like.fn) return fail("bpm_eval_device_likelihood: no device likelihood installed (bpm_set_device_likelihood)");
    if (s->proposed) return fail("bpm_eval_device_likelihood: a half generation is open (bpm_propose ... without its commit)");
    if (n <= 0) return 0;
    if (!X || !out) return fail("bpm_eval_device_likelihood: null argument");
    DevTemp<double> bX, bO;
    CK(bX.alloc((size_t)n * s->ld, "bpm_eval_device_likelihood", "the rows"));
    CK(bO.alloc((size_t)n));
    HIPCK(hipMemsetAsync(bX.p, 0, (size_t)n * s->ld * sizeof(double), s->stream));
    HIPCK(hipMemcpy2DAsync(bX.p, s->ld * sizeof(double), X, s->dim * sizeof(double), s->dim * sizeof(double), n, hipMemcpyHostToDevice, s->stream));
    CK(user_ll_launch(s, bX.p, nullptr, (uint32_t)n, bO.p));
    HIPCK(hipMemcpyAsync(out, bO.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

// which form of the device likelihood runs: *fused = 1 the update kernel compiled around it (one launch per half generation), 0 the three-kernel form
// (then `why`, if given, says why: up to why_cap - 1 characters); error when no device likelihood is installed
extern "C" int bpm_get_device_likelihood_info(bpm_handle_t s, int32_t* fused, char* why, int64_t why_cap) {
    CK(check_handle(s));
    if (!s->like.fn) return fail("bpm_get_device_likelihood_info: no device likelihood installed (bpm_set_device_likelihood)");
    if (fused) *fused = s->like.fused.fn ? 1 : 0;
    bpm::copy_text(s->like.why, why, why_cap);
    return 0;
}

extern "C" int bpm_refresh_device_loglike(bpm_handle_t s) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->like.fn) return fail("bpm_refresh_device_loglike: no device likelihood installed (bpm_set_device_likelihood)");
    return user_refresh_ll(s);
}

// ---- posterior summaries of a caller's derived quantities (derived.h; bipymc_amd/derived.py merges the ranks and finishes mean and sd) ------
// What the reference's fitting scripts do on the host with param_est(n_burn)[2] (examples/ex_exp_fit.py:197-202: c_0 / c_inf per sample, its
// mean and standard deviation; :176-192: the fitted model at every sample), taken where the history lives.
static int check_n_out(const char* who, int32_t n_out) {
    if (n_out < 1 || n_out > DERIVE_MAX_OUT)
        return fail(std::string(who) + ": n_out must be 1 ... " + std::to_string(DERIVE_MAX_OUT) + " (got " + std::to_string(n_out) + ")");
    return 0;
}

extern "C" int bpm_check_device_function(const char* hip_source, int32_t n_out, const char* arch, char* log, int64_t log_cap) {
    return check_source("bpm_check_device_function", hip_source, arch, log, log_cap, [&] { return check_n_out("bpm_check_device_function", n_out); },
                        [&](const char* a, std::vector<char>& code) { return bpm::compile_device_function(hip_source, a, bpm_embedded, N_EMBEDDED, code); });
}

extern "C" int bpm_set_device_function(bpm_handle_t s, const char* hip_source, int32_t n_out, const double* params, int32_t n_params) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!hip_source || n_params < 0 || (n_params > 0 && !params)) return fail("bpm_set_device_function: bad argument");
    CK(check_n_out("bpm_set_device_function", n_out));
    // (install_function) the same source bytes and n_out: the parameters only
    const bool same = s->derived.fn && s->derived.n_out == n_out && s->derived.src == hip_source;
    return install_function(s->stream, s->derived, same, params, n_params, [&](DerivedFunction& next) {
        CK(compile_and_load("bpm_set_device_function", s->cfg.device, [&](const std::string& arch, std::vector<char>& code) {
            return bpm::compile_device_function(hip_source, arch, bpm_embedded, N_EMBEDDED, code); }, next.mod, {{"bpm_derive_rows", &next.fn}, {"bpm_derive_fill", &next.fill}}));
        next.src = hip_source;
        next.n_out = n_out;
        return 0;
    });
}

// tile and grid of a launch of the installed function's kernels over `rows` rows of s: rows per tile R, the LDS strides, the dynamic LDS, the workgroups
static int derive_launch_shape(const bpm_sampler* s, uint64_t rows, const char* who, uint32_t& R, uint32_t& ldp, uint32_t& ldo, uint32_t& lds, uint64_t* parts) {
    // BPM_DERIVE_LDS_KB (16 ... 60; read at every call: tools/derived_time.py switches it): the LDS budget of a workgroup's tiles (A/B)
    uint32_t budget = (uint32_t)DERIVE_LDS_BYTES;
    if (const char* kb = getenv("BPM_DERIVE_LDS_KB")) budget = (uint32_t)std::min(std::max(atoi(kb), 16), DERIVE_LDS_BYTES / 1024) * 1024u;
    derive_tile(s->dim, (uint32_t)s->derived.n_out, budget, R, ldp, ldo, lds);
    return rows_grid(rows, 1, R, who, parts);
}

// Over this rank's super-chain rows >= n_burn (bpm_reduce_moments' selection: a partial first generation by chain index), per output m of
// the installed function: counts = [2][n_out]: how many values are finite | NaN; sums = [5][n_out]: shift | S1 | S2 | min | max (bpm_trace_bins'
// meaning).  *n_rows: the window's local rows, *n_first of them in a partial first generation (0: whole generations only).  values (may be
// null): values[r * n_out + m] for the window's local rows r in order, at most values_cap doubles.  Keeps no state; every buffer is temporary.
extern "C" int bpm_derive(bpm_handle_t s, int64_t n_burn, int64_t* counts, double* sums, int64_t* n_rows, int64_t* n_first, double* values,
                          int64_t values_cap) {
    const std::string who = "bpm_derive";
    RowWindow w;
    CK(open_window(s, who, !counts || !sums || !n_rows || !n_first, n_burn,
                   [&] { return s->derived.fn ? 0 : fail(who + ": no device function installed (bpm_set_device_function)"); }, w));
    const uint32_t n_out = (uint32_t)s->derived.n_out;
    *n_rows = (int64_t)w.rows;
    *n_first = (int64_t)(w.rows % s->n_local);
    std::fill(counts, counts + 2 * (size_t)n_out, (int64_t)0);
    std::fill(sums, sums + 5 * (size_t)n_out, 0.0);
    std::fill(sums + 3 * (size_t)n_out, sums + 4 * (size_t)n_out, HUGE_VAL);
    std::fill(sums + 4 * (size_t)n_out, sums + 5 * (size_t)n_out, -HUGE_VAL);
    if (w.rows == 0) return 0;
    CK(check_values(who, values, values_cap, w, n_out, "outputs"));
    uint32_t R = 0, ldp = 0, ldo = 0, lds = 0;
    uint64_t parts = 1;
    CK(derive_launch_shape(s, w.rows, who.c_str(), R, ldp, ldo, lds, &parts));
    const auto launch = [&](double* rec, uint64_t n_rec, double* v) {
        return ModuleLaunch<bpm::DeriveRowsKernel>::on(s->stream, s->derived.fn, (unsigned)parts, DERIVE_THREADS, lds, s->hist, s->llhist, s->ld, (int)s->dim, w.lo, w.hi,
                                                       s->derived.params.p, n_out, R, ldp, ldo, rec, n_rec, v); };
    const auto fold = [&](const double* rec, double* folded) {
        hipLaunchKernelGGL(tr_fold_kernel, dim3((unsigned)((n_out + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, s->stream, rec, (uint32_t)parts, n_out,
                           (uint64_t)n_out, (uint32_t)TR_F_BINS, folded); };
    std::vector<double> h((size_t)TR_F_BINS * n_out);
    CK(window_records(s, who, w, parts, "workgroups", TR_F_BINS, n_out, "outputs", values, launch, fold, h.data()));
    const int count_f[2] = {TR_N, TR_NAN}, sum_f[5] = {TR_C, TR_S1, TR_S2, TR_MIN, TR_MAX};
    for (uint32_t m = 0; m < n_out; ++m) {
        for (int f = 0; f < 2; ++f) std::memcpy(&counts[(size_t)f * n_out + m], &h[(size_t)count_f[f] * n_out + m], 8);
        for (int f = 0; f < 5; ++f) sums[(size_t)f * n_out + m] = h[(size_t)sum_f[f] * n_out + m];
    }
    return 0;
}

// ---- WAIC's ingredients per datum of a caller's data (pointwise.h, pointwise_rows.h; bipymc_amd/pointwise.py merges the ranks and finishes) --------
// The reference has no such statistic: its fitting scripts sum a log density over their data points inside ln_like_fn (examples/ex_line_fit.py:63-67);
// here one term of that sum is the caller's, and its log-sum-exp and moments over the draws are taken where the history lives.
static int check_pointwise_w(const char* who, int32_t w) {
    if (w < 1 || w > bpm::PW_MAX_W) return fail(std::string(who) + ": w must be 1 ... " + std::to_string(bpm::PW_MAX_W) + " (got " + std::to_string(w) + ")");
    return 0;
}

extern "C" int bpm_check_pointwise(const char* hip_source, int32_t w, const char* arch, char* log, int64_t log_cap) {
    return check_source("bpm_check_pointwise", hip_source, arch, log, log_cap, [&] { return check_pointwise_w("bpm_check_pointwise", w); },
                        [&](const char* a, std::vector<char>& code) { return bpm::compile_pointwise(hip_source, w, a, bpm_embedded, N_EMBEDDED, code); });
}

extern "C" int bpm_set_pointwise(bpm_handle_t s, const char* hip_source, const double* params, int32_t n_params, const double* data, int64_t n_data, int32_t w,
                                 int32_t* reused) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!hip_source || n_params < 0 || (n_params > 0 && !params)) return fail("bpm_set_pointwise: bad argument");
    CK(check_pointwise_w("bpm_set_pointwise", w));
    if (!data || n_data < 1 || n_data > (int64_t)0x7fffffff) return fail("bpm_set_pointwise: data must be (n_data, w) with 1 <= n_data < 2^31");
    const size_t n_val = (size_t)n_data * (size_t)w;
    // (install_function) the same source bytes, w and data: the parameters only -- and PSIS-LOO's module, which leaves with a rebuild, stays
    const PointwiseFunction& cur = s->pointwise;
    const bool same = cur.fn && cur.w == w && cur.n_data == n_data && cur.src == hip_source && std::memcmp(cur.data_h.data(), data, n_val * sizeof(double)) == 0;
    if (reused) *reused = same ? 1 : 0;
    return install_function(s->stream, s->pointwise, same, params, n_params, [&](PointwiseFunction& next) {
        CK(compile_and_load("bpm_set_pointwise", s->cfg.device, [&](const std::string& arch, std::vector<char>& code) {
            return bpm::compile_pointwise(hip_source, w, arch, bpm_embedded, N_EMBEDDED, code); }, next.mod, {{"bpm_pointwise_rows", &next.fn}}));
        next.src = hip_source;
        next.w = w;
        next.n_data = n_data;
        next.data_h.assign(data, data + n_val);
        CK(next.data.alloc(n_val, "bpm_set_pointwise", "the data"));
        HIPCK(hipMemcpyAsync(next.data.p, data, n_val * sizeof(double), hipMemcpyHostToDevice, s->stream));
        return 0;
    });
}

extern "C" int bpm_pointwise_layout(int32_t d, int32_t w, int64_t n_rows, int64_t n_data, int64_t* out) {
    if (!out || d < 1 || n_rows < 0 || n_data < 1 || n_data > (int64_t)0x7fffffff) return fail("bpm_pointwise_layout: bad argument");
    CK(check_pointwise_w("bpm_pointwise_layout", w));
    const bpm::PointwiseLayout L = bpm::pointwise_layout((uint32_t)d, (uint64_t)n_rows, (uint64_t)n_data);
    out[0] = bpm::PW_THREADS; out[1] = L.R; out[2] = (int64_t)L.parts; out[3] = (int64_t)L.chunk;
    return 0;
}

// Over this rank's super-chain rows >= n_burn (bpm_reduce_moments' selection: a partial first generation by chain index), per datum i of the installed
// function's data: records = [PW_FIELDS][n_data] (pointwise_rows.h), counts as 64-bit words.  *n_rows: the window's local rows, *n_first of them in a
// partial first generation.  values (may be null): values[r * n_data + i] for the window's local rows r in order, at most values_cap doubles.
// Keeps no state; every buffer but the function's own data and parameters is temporary.
extern "C" int bpm_pointwise(bpm_handle_t s, int64_t n_burn, double* records, int64_t* n_rows, int64_t* n_first, double* values, int64_t values_cap) {
    const std::string who = "bpm_pointwise";
    RowWindow w;
    CK(open_window(s, who, !records || !n_rows || !n_first, n_burn,
                   [&] { return s->pointwise.fn ? 0 : fail(who + ": no pointwise function installed (bpm_set_pointwise)"); }, w));
    const PointwiseFunction& f = s->pointwise;
    const uint64_t n_data = (uint64_t)f.n_data;
    *n_rows = (int64_t)w.rows;
    *n_first = (int64_t)(w.rows % s->n_local);
    std::memset(records, 0, (size_t)PW_FIELDS * n_data * sizeof(double));
    if (w.rows == 0) return 0;
    CK(check_values(who, values, values_cap, w, n_data, "data points"));
    const bpm::PointwiseLayout L = bpm::pointwise_layout(s->dim, w.rows, n_data);
    if (L.parts * L.n_tiles >= (1ull << 31)) return fail(who + ": window too large");
    const auto launch = [&](double* rec, uint64_t n_rec, double* v) {
        return ModuleLaunch<bpm::PointwiseRowsKernel>::on(s->stream, f.fn, (unsigned)(L.parts * L.n_tiles), PW_THREADS, L.lds_bytes, s->hist, s->ld, (int)s->dim, w.lo, w.hi,
                                                          L.chunk, (unsigned)L.n_tiles, f.params.p, f.data.p, (unsigned)n_data, L.R, L.ldp, rec, n_rec, v); };
    const auto fold = [&](const double* rec, double* folded) {
        hipLaunchKernelGGL(pw_fold_kernel, dim3((unsigned)L.n_tiles), dim3(PW_THREADS), 0, s->stream, rec, (uint32_t)L.parts, n_data, folded); };
    return window_records(s, who, w, L.parts, "parts", PW_FIELDS, n_data, "data points", values, launch, fold, records);
}

// ---- a second handle as the destination of a history built from the first (bpm_derive_history, bpm_rank_history) -------------------------
// The pair itself: two live handles, drained, on one device (made current).  `dim_hint`: what the refusal of src == dst recommends.
static int second_handle_pair(const std::string& who, bpm_handle_t src, bpm_handle_t dst, const char* dim_hint) {
    if (!src || !dst) return fail(who + ": null handle");
    if (src == dst) return fail(who + ": the destination is the source itself (create a second handle with " + dim_hint + ")");
    CK(check_handle(src));
    CK(check_handle(dst));
    if (src->cfg.device != dst->cfg.device)
        return fail(who + ": source and destination are on different devices (" + std::to_string(src->cfg.device) + " and " +
                    std::to_string(dst->cfg.device) + ")");
    CK(set_device(src));
    return 0;
}
static int second_handle_single_rank(const std::string& who, const bpm_sampler* src, const bpm_sampler* dst) {
    if (src->world != 1 || dst->world != 1)
        return fail(who + ": single rank only (world_size " + std::to_string(src->world) + " and " + std::to_string(dst->world) + ")");
    return 0;
}
// The destination can take it: a history-keeping host-callback handle of `dim` coordinates (`dim_of`: whose dim that is) and src's chains, nothing open.
static int second_handle_fits(const std::string& who, const bpm_sampler* src, const bpm_sampler* dst, uint32_t dim, const char* dim_of) {
    if (!dst->cfg.keep_history) return fail(who + ": the destination needs keep_history=True");
    if (dst->cfg.target_id != BPM_TARGET_HOST_CALLBACK) return fail(who + ": the destination must have the host-callback target");
    if (dst->dim != dim) return fail(who + ": the destination has dim " + std::to_string(dst->dim) + "; " + dim_of + " " + std::to_string(dim));
    if (dst->N != src->N) return fail(who + ": the destination has n_chains " + std::to_string(dst->N) + "; the source has " + std::to_string(src->N));
    if (dst->proposed) return fail(who + ": the destination has proposals that are not committed");
    return 0;
}

// A DERIVED HISTORY IS A HISTORY: the installed function of `src` over every resident row of src, written into the history buffer of `dst`, a
// second, ordinary handle with dim = n_out -- whose bpm_reduce_moments ... bpm_trace_chains (and bpm_derive) then serve the derived quantities
// with their own scratch, sized by their own ld, and their own state for bpm_reduce_moments' shift.  dst comes out as bpm_set_history leaves a
// handle: rows in chain order, the state = the last row, the ln-likes = src's.  Every check runs before any launch; nothing src's sampler reads
// is written (its history is put into chain order, as bpm_get_history does).
extern "C" int bpm_derive_history(bpm_handle_t src, bpm_handle_t dst) {
    const char* who = "bpm_derive_history";
    CK(second_handle_pair(who, src, dst, "dim = n_out"));
    if (!src->derived.fill) return fail(std::string(who) + ": no device function installed on the source (bpm_set_device_function)");
    CK(require_resident_history(src, who));
    CK(second_handle_single_rank(who, src, dst));
    const uint32_t n_out = (uint32_t)src->derived.n_out;
    CK(second_handle_fits(who, src, dst, n_out, "the installed function has n_out"));
    const int64_t rows = src->hist_rows;
    const uint64_t n = (uint64_t)rows * src->n_local;      // local rows of both
    uint32_t R = 0, ldp = 0, ldo = 0, lds = 0;
    uint64_t parts = 1;
    CK(derive_launch_shape(src, n, who, R, ldp, ldo, lds, &parts));
    size_t mem_free = 0, mem_total = 0;
    uint64_t need = 0;
    HIPCK(hipMemGetInfo(&mem_free, &mem_total));
    CK(history_growth_bytes(dst, rows, who, "derived", mem_free, &need));
    CK(normalize_history(src, 0, src->hist_rows));
    CK(ensure_history(dst, rows));
    HIPCK(ModuleLaunch<bpm::DeriveFillKernel>::on(src->stream, src->derived.fill, (unsigned)parts, DERIVE_THREADS, lds, src->hist, src->llhist, src->ld,
                                                  (int)src->dim, (unsigned long long)n, src->derived.params.p, n_out, R, ldp, ldo, dst->hist, dst->ld));
    const size_t row_d = (size_t)dst->n_local * dst->ld;
    const double* ll_last = src->llhist + (size_t)(rows - 1) * src->n_local;
    HIPCK(hipMemcpyAsync(dst->llhist, src->llhist, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, src->stream));
    // the state and the ln-like cache bpm_set_history + bpm_set_loglike leave behind: the last row (bpm_reduce_moments' shift: a value of the data)
    HIPCK(hipMemcpyAsync(dst->G, dst->hist + (size_t)(rows - 1) * row_d, row_d * sizeof(double), hipMemcpyDeviceToDevice, src->stream));
    HIPCK(hipMemcpyAsync(dst->ll, ll_last, (size_t)dst->n_local * sizeof(double), hipMemcpyDeviceToDevice, src->stream));
    history_installed(dst, rows);
    HIPCK(hipStreamSynchronize(src->stream));
    return 0;
}

// ---- pooled ranks of the history (ranks.h; bipymc_amd/rank_diagnostics.py drives the fills) ---------------------------------------------
// segment kk of the sort = column kk of the batch: keys [kk * S, (kk + 1) * S)
struct RankSegment {
    uint32_t S;
    __host__ __device__ uint32_t operator()(uint32_t kk) const { return kk * S; }
};

// the segmented radix sort of bc columns of S keys each (tmp == nullptr: only its temporaries' size into *tmp_bytes); on the HIP stream
static hipError_t rank_sort(void* tmp, size_t* tmp_bytes, unsigned long long* in, unsigned long long* out, uint32_t bc, uint32_t S, hipStream_t st) {
    auto seg = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), RankSegment{S});
    return rocprim::segmented_radix_sort_keys(tmp, *tmp_bytes, in, out, bc * S, bc, seg, seg + 1, 0u, 64u, st);
}

// ---- PSIS-LOO per datum (pointwise_tail.h: the exact tail and the body's log-sum-exp; psis.h: fit and finish; bipymc_amd/pointwise.py) ------------
// The reference has no such statistic.  bpm_loo_kept: the size K of a datum's kept set for a window of n_rows draws (psis.h: psis_kept).
extern "C" int64_t bpm_loo_kept(int64_t n_rows, double r_eff) {
    if (n_rows < 0 || !(r_eff > 0.0) || !std::isfinite(r_eff)) return -1;
    return (int64_t)bpm::psis_kept((uint64_t)n_rows, r_eff);
}

// the scratch budget of a call: BPM_LOO_SCRATCH_MB, or a quarter of the free memory (read at every call)
static uint64_t loo_budget(size_t mem_free) {
    if (const char* mb = getenv("BPM_LOO_SCRATCH_MB")) return (uint64_t)std::max(atoll(mb), 0ll) << 20;
    return (uint64_t)mem_free / 4;
}
static int loo_plan(const std::string& who, uint32_t d, uint64_t n_rows, uint64_t n_data, uint64_t k_max, uint64_t budget, bool from_env_or_free, size_t mem_free,
                    bpm::PointwiseLayout* P, bpm::LooLayout* A) {
    *P = bpm::pointwise_layout(d, n_rows, n_data);
    *A = bpm::loo_layout(*P, n_rows, k_max, bpm::psis_work(k_max), budget);
    if (n_rows > 0 && A->too_many_keys)
        return fail(who + ": kept sets of " + std::to_string((unsigned long long)k_max) + " values are too large: one tile of " + std::to_string(bpm::PW_THREADS) +
                    " data must hold fewer than 2^31 keys for the sort (raise r_eff towards 1, shorten the window with n_burn, or thin the history)");
    if (n_rows > 0 && !A->fits)
        return fail(who + ": the kept sets of one tile of " + std::to_string(bpm::PW_THREADS) + " data (" + std::to_string((unsigned long long)k_max) +
                    " of " + std::to_string((unsigned long long)n_rows) + " draws each) need " + std::to_string((unsigned long long)A->per_tile_bytes) +
                    " bytes of scratch; the budget is " + std::to_string((unsigned long long)budget) + " bytes" +
                    (from_env_or_free ? " (BPM_LOO_SCRATCH_MB; by default a quarter of the free device memory: " + std::to_string(mem_free >> 20) + " MiB are free)" : std::string()) +
                    ": raise r_eff towards 1, shorten the window with n_burn, or thin the history");
    if (n_rows > 0 && (A->parts * A->batch_tiles >= (1ull << 31) || P->parts * A->batch_tiles >= (1ull << 31) || 2 * k_max >= (1ull << 32)))
        return fail(who + ": window too large");
    return 0;
}

extern "C" int bpm_loo_layout(int32_t d, int32_t w, int64_t n_rows, int64_t n_data, int64_t k_max, int64_t budget_bytes, int64_t* out) {
    if (!out || d < 1 || n_rows < 0 || n_data < 1 || n_data > (int64_t)0x7fffffff || k_max < 1 || k_max > std::max<int64_t>(n_rows, 1) || budget_bytes < 0)
        return fail("bpm_loo_layout: bad argument");
    CK(check_pointwise_w("bpm_loo_layout", w));
    bpm::PointwiseLayout P;
    bpm::LooLayout A;
    CK(loo_plan("bpm_loo_layout", (uint32_t)d, (uint64_t)n_rows, (uint64_t)n_data, (uint64_t)k_max, (uint64_t)budget_bytes, false, 0, &P, &A));
    out[0] = bpm::PW_THREADS; out[1] = P.R; out[2] = (int64_t)A.parts; out[3] = (int64_t)A.chunk; out[4] = (int64_t)A.batch_tiles; out[5] = (int64_t)A.batches;
    out[6] = (int64_t)P.parts; out[7] = (int64_t)P.chunk;
    return 0;
}

// Over this rank's super-chain rows >= n_burn (bpm_pointwise's window; single rank), per datum i of the installed function's data with relative
// efficiency r_eff[i]: records = [LOO_FIELDS][n_data] (psis.h).  tails (may be null): tails[i * k_max + j], j < kept_i, the kept values ascending, k_max the
// largest kept set of the call (stats[1]).  stats[12]: rows | k_max | stage A's parts | data batches | the most compactions a workgroup of stage A made |
// stage B's parts | stage B's rows per part | the scratch budget in bytes | the microseconds of stage A (selection, merge, sort), of B and of C on the
// device, summed over the batches (event pairs on the stream) | 1 if this call compiled the module of stages A and B, 0 if it was kept.  Every check
// and the plan come before this call compiles or allocates anything (the function installed by bpm_set_pointwise is there already).
extern "C" int bpm_loo(bpm_handle_t s, int64_t n_burn, const double* r_eff, double* records, double* tails, int64_t tails_cap, int64_t* stats) {
    const std::string who = "bpm_loo";
    RowWindow w;
    CK(open_window(s, who, !r_eff || !records || !stats, n_burn, [&] {
        if (s->world != 1) return fail(who + ": single rank only (world_size " + std::to_string(s->world) + ")");
        return s->pointwise.fn ? 0 : fail(who + ": no pointwise function installed (bpm_set_pointwise)"); }, w));
    PointwiseFunction& f = s->pointwise;
    const uint64_t lo = w.lo, hi = w.hi, rows = w.rows, n_data = (uint64_t)f.n_data;
    std::memset(records, 0, (size_t)bpm::LOO_FIELDS * n_data * sizeof(double));
    std::memset(stats, 0, 12 * sizeof(int64_t));
    stats[0] = (int64_t)rows;
    if (rows == 0) return 0;
    std::vector<unsigned int> keep_h((size_t)n_data);
    uint64_t k_max = 0;
    for (uint64_t i = 0; i < n_data; ++i) {
        if (!(r_eff[i] > 0.0) || !std::isfinite(r_eff[i])) return fail(who + ": r_eff must be finite and > 0 (datum " + std::to_string((unsigned long long)i) + ")");
        const uint64_t K = bpm::psis_kept(rows, r_eff[i]);
        if (K >= (1ull << 31)) return fail(who + ": window too large");
        keep_h[(size_t)i] = (unsigned int)K;
        k_max = std::max(k_max, K);
    }
    if (tails && (tails_cap < 0 || (uint64_t)tails_cap < n_data * k_max))
        return fail(who + ": tails holds " + std::to_string((long long)tails_cap) + " doubles; " + std::to_string((unsigned long long)n_data) + " data x " +
                    std::to_string((unsigned long long)k_max) + " kept values are needed");
    size_t mem_free = 0, mem_total = 0;
    HIPCK(hipMemGetInfo(&mem_free, &mem_total));
    const uint64_t budget = loo_budget(mem_free);
    bpm::PointwiseLayout P;
    bpm::LooLayout A;
    CK(loo_plan(who, s->dim, rows, n_data, k_max, budget, true, mem_free, &P, &A));
    const uint64_t nbt = A.batch_tiles, n_cols = nbt * bpm::PW_THREADS, n_wg = A.parts * nbt, ws_stride = bpm::psis_work(k_max);
    size_t sort_bytes = 0;
    HIPCK(rank_sort(nullptr, &sort_bytes, nullptr, nullptr, (uint32_t)n_cols, (uint32_t)k_max, s->stream));
    if (!f.tail_fn) {      // (the first call with this source: stages A and B are compiled around it)
        Module mod;
        hipFunction_t a = nullptr, b = nullptr, c = nullptr;
        CK(compile_and_load(who, s->cfg.device, [&](const std::string& arch, std::vector<char>& code) {
            return bpm::compile_pointwise_tail(f.src, f.w, arch, bpm_embedded, N_EMBEDDED, code); }, mod,
                            {{"bpm_pointwise_tail", &a}, {"bpm_pointwise_tail_final", &b}, {"bpm_pointwise_body", &c}}));
        f.tail_mod = std::move(mod);
        f.tail_fn = a; f.tail_final_fn = b; f.body_fn = c;
        stats[11] = 1;
    }
    DevTemp<unsigned int> d_keep, d_cnt, d_bad, d_ncomp, d_nkept, d_nbad;
    DevTemp<unsigned long long> d_buf, d_keys;
    DevTemp<double> d_ws, d_cut, d_body, d_out;
    DevTemp<char> d_sort;
    CK(d_keep.alloc((size_t)n_data, who.c_str(), "the kept-set sizes"));
    CK(d_buf.alloc((size_t)(n_wg * A.cap * bpm::PW_THREADS), who.c_str(), "the candidate buffers of " + std::to_string((unsigned long long)n_wg) + " workgroups"));
    CK(d_cnt.alloc((size_t)(n_wg * bpm::PW_THREADS)));
    CK(d_bad.alloc((size_t)(n_wg * bpm::PW_THREADS)));
    CK(d_ncomp.alloc((size_t)n_wg));
    CK(d_nkept.alloc((size_t)n_cols));
    CK(d_nbad.alloc((size_t)n_cols));
    CK(d_keys.alloc((size_t)(2 * n_cols * k_max), who.c_str(), "the kept values of " + std::to_string((unsigned long long)n_cols) + " data (the sort's in and out)"));
    CK(d_sort.alloc(std::max<size_t>(sort_bytes, 1), who.c_str(), "the sort's temporaries"));
    CK(d_ws.alloc((size_t)(n_cols * ws_stride), who.c_str(), "the fit's work space"));
    CK(d_cut.alloc((size_t)n_cols));
    CK(d_body.alloc((size_t)(3 * P.parts * n_cols), who.c_str(), "the body records of " + std::to_string((unsigned long long)P.parts) + " parts"));
    CK(d_out.alloc((size_t)bpm::LOO_FIELDS * n_data));
    // ---- nothing was launched so far ----
    CK(normalize_history(s, (int64_t)(lo / s->n_local), s->hist_rows));
    HIPCK(hipMemcpyAsync(d_keep.p, keep_h.data(), (size_t)n_data * sizeof(unsigned int), hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemsetAsync(d_out.p, 0, (size_t)bpm::LOO_FIELDS * n_data * sizeof(double), s->stream));
    unsigned long long* k_in = d_keys.p;
    unsigned long long* k_out = d_keys.p + (size_t)(n_cols * k_max);
    std::vector<unsigned int> ncomp_h((size_t)n_wg);
    std::vector<double> tails_h;
    unsigned int most = 0;
    struct Events {      // (destroyed on every way out)
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    for (hipEvent_t& x : ev.e) HIPCK(hipEventCreate(&x));
    double us[3] = {0.0, 0.0, 0.0};
    for (uint64_t b = 0; b < A.batches; ++b) {
        const uint64_t tile0 = b * nbt, nt = std::min<uint64_t>(nbt, P.n_tiles - tile0), cols = nt * bpm::PW_THREADS;
        const uint64_t i0 = tile0 * bpm::PW_THREADS, n_live = std::min<uint64_t>(cols, n_data - i0);
        HIPCK(hipEventRecord(ev.e[0], s->stream));
        HIPCK(ModuleLaunch<bpm::PointwiseTailKernel>::on(s->stream, f.tail_fn, (unsigned)(A.parts * nt), bpm::PW_THREADS, P.lds_bytes + bpm::PT_HIST_BYTES, s->hist, s->ld,
                                                         (int)s->dim, lo, hi, A.chunk, (unsigned)nt, (unsigned)tile0, f.params.p, f.data.p, (unsigned)n_data, P.R, P.ldp,
                                                         P.lds_bytes / 8u, d_keep.p, (unsigned)A.cap, d_buf.p, d_cnt.p, d_bad.p, d_ncomp.p));
        HIPCK(ModuleLaunch<bpm::PointwiseTailFinalKernel>::on(s->stream, f.tail_final_fn, (unsigned)nt, bpm::PW_THREADS, 0, (unsigned)nt, (unsigned)tile0, (unsigned)A.parts,
                                                              (unsigned)n_data, d_keep.p, (unsigned)A.cap, (unsigned)k_max, d_buf.p, d_cnt.p, d_bad.p, k_in, d_nkept.p,
                                                              d_nbad.p));
        size_t t = sort_bytes;      // (the temporaries of a full batch hold those of the last, partial one)
        HIPCK(rank_sort(d_sort.p, &t, k_in, k_out, (uint32_t)cols, (uint32_t)k_max, s->stream));
        HIPCK(hipEventRecord(ev.e[1], s->stream));
        hipLaunchKernelGGL(pw_tail_values_kernel, dim3((unsigned)cols), dim3(bpm::PSIS_THREADS), 0, s->stream, k_out, (uint32_t)k_max, cols, (const uint32_t*)d_nkept.p,
                           (const uint32_t*)d_nbad.p, d_cut.p);
        HIPCK(hipGetLastError());
        const uint64_t n_rec = P.parts * cols;
        HIPCK(ModuleLaunch<bpm::PointwiseBodyKernel>::on(s->stream, f.body_fn, (unsigned)(P.parts * nt), bpm::PW_THREADS, P.lds_bytes, s->hist, s->ld, (int)s->dim, lo, hi,
                                                         P.chunk, (unsigned)nt, (unsigned)tile0, f.params.p, f.data.p, (unsigned)n_data, P.R, P.ldp, d_cut.p, d_body.p,
                                                         n_rec));
        HIPCK(hipEventRecord(ev.e[2], s->stream));
        hipLaunchKernelGGL(pw_psis_kernel, dim3((unsigned)n_live), dim3(bpm::PSIS_THREADS), 0, s->stream, (const double*)k_out, (uint32_t)k_max, cols,
                           (const uint32_t*)d_nkept.p, (const uint32_t*)d_nbad.p, (const double*)d_body.p, (uint32_t)P.parts, d_ws.p, ws_stride, i0, n_data, d_out.p);
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(ev.e[3], s->stream));
        HIPCK(hipMemcpyAsync(ncomp_h.data(), d_ncomp.p, (size_t)(A.parts * nt) * sizeof(unsigned int), hipMemcpyDeviceToHost, s->stream));
        if (tails) HIPCK(hipMemcpyAsync(tails + (size_t)(i0 * k_max), k_out, (size_t)(n_live * k_max) * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        for (uint64_t q = 0; q < A.parts * nt; ++q) most = std::max(most, ncomp_h[(size_t)q]);
        for (int k = 0; k < 3; ++k) {
            float ms = 0.0f;
            HIPCK(hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
            us[k] += 1e3 * (double)ms;
        }
    }
    HIPCK(hipMemcpyAsync(records, d_out.p, (size_t)bpm::LOO_FIELDS * n_data * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    stats[1] = (int64_t)k_max; stats[2] = (int64_t)A.parts; stats[3] = (int64_t)A.batches; stats[4] = (int64_t)most; stats[5] = (int64_t)P.parts;
    stats[6] = (int64_t)P.chunk; stats[7] = (int64_t)budget;
    for (int k = 0; k < 3; ++k) stats[8 + k] = (int64_t)(us[k] + 0.5);
    return 0;
}

// ---- the one batch loop of whatever reads sorted columns: bpm_rank_history's sorted kinds (the consumer scores) and bpm_hdi (it scans) ---
// rank_window_checks: S and the order statistics' positions; rank_batches_plan: the batch the scratch budget holds and every allocation;
// rank_batches_run: per batch of columns the keys, the sort, the picks, then consume(k0, b, kw, n_tiles, nby, sorted) -- the batch's first
// column and width, rk_keys_kernel's launch shape over it, and its sorted keys [b][S].  Nothing is launched before run.
struct RankBatches {
    uint32_t S = 0, dim = 0, bc = 0;
    int32_t n_pos = 0;
    size_t tmp_bytes = 0;
    DevTemp<unsigned long long> keys, d_pos;
    DevTemp<unsigned char> tmp;
    DevTemp<double> d_os;
};

static int rank_window_checks(const std::string& who, uint64_t S64, const char* verb, int32_t n_pos, const int64_t* pos) {
    if (S64 >= (1ull << 31))
        return fail(who + ": the window holds " + std::to_string((unsigned long long)S64) + " values per coordinate; fewer than 2^31 can be " + verb);
    for (int32_t j = 0; j < n_pos; ++j)
        if (pos[j] < 0 || (uint64_t)pos[j] >= S64)
            return fail(who + ": order statistic " + std::to_string((long long)pos[j]) + " is outside [0, " + std::to_string((unsigned long long)S64) + ")");
    return 0;
}

// the batch: as many columns as the scratch budget holds (keys in | keys out | the sort's temporaries), batch * S < 2^31.
// The sort gives a column of this length to ONE workgroup, so the columns of a batch are its whole parallelism: at cfg2's shape with 1000
// generations a z fill takes 24.7 / 6.8 / 2.1 / 1.0 s with batches of 1 / 4 / 16 / 64 columns (profiles/rank_diagnostics_cfg2.txt).  Hence
// the default budget: a quarter of the free memory.  BPM_RANK_SCRATCH_MB: the budget; BPM_RANK_BATCH_COLS: the batch itself (tests, A/B;
// both read at every call)
static int rank_batches_plan(RankBatches& rb, const std::string& who, bpm_sampler* src, uint32_t S, size_t mem_free, int32_t n_pos) {
    const uint32_t dim = src->dim;
    rb.S = S; rb.dim = dim; rb.n_pos = n_pos;
    uint64_t budget = mem_free / 4;
    if (const char* mb = getenv("BPM_RANK_SCRATCH_MB")) budget = (uint64_t)std::max(atoll(mb), 0ll) << 20;
    const uint32_t bc_max = std::min<uint32_t>(dim, (uint32_t)(((1ull << 31) - 1) / S));
    auto need_of = [&](uint32_t b, uint64_t* need) -> int {
        size_t t = 0;
        HIPCK(rank_sort(nullptr, &t, nullptr, nullptr, b, S, src->stream));
        rb.tmp_bytes = t;
        *need = 2ull * b * S * sizeof(unsigned long long) + t;
        return 0;
    };
    uint64_t need = 0;
    uint32_t bc = 0;
    const char* forced = getenv("BPM_RANK_BATCH_COLS");
    if (forced && atoi(forced) > 0) {
        bc = std::min<uint32_t>((uint32_t)atoi(forced), bc_max);
        CK(need_of(bc, &need));
    } else {
        bc = (uint32_t)std::min<uint64_t>(bc_max, std::max<uint64_t>(1, budget / (16ull * S)));
        CK(need_of(bc, &need));
        while (bc > 1 && need > budget) {
            bc = std::max<uint32_t>(1, std::min<uint32_t>(bc - 1, (uint32_t)((uint64_t)bc * budget / need)));
            CK(need_of(bc, &need));
        }
        if (need > budget)
            return fail(who + ": sorting one column of " + std::to_string(S) + " keys needs " + std::to_string((unsigned long long)need) +
                        " bytes of scratch (keys in, keys out and the sort's temporaries); the budget is " + std::to_string((unsigned long long)budget) +
                        " bytes (BPM_RANK_SCRATCH_MB; by default a quarter of the free device memory: " + std::to_string(mem_free >> 20) +
                        " MiB are free)");
    }
    rb.bc = bc;
    const std::string what = "the scratch of " + std::to_string(bc) + " columns of " + std::to_string(S) + " keys";
    CK(rb.keys.alloc(2 * (size_t)bc * S, who.c_str(), what + " (keys in, keys out)"));
    CK(rb.tmp.alloc(std::max<size_t>(rb.tmp_bytes, 1), who.c_str(), what + " (the sort's temporaries)"));
    if (n_pos > 0) {
        CK(rb.d_os.alloc((size_t)n_pos * dim));
        CK(rb.d_pos.alloc((size_t)n_pos));
    }
    return 0;
}

template <class Consume>
static int rank_batches_run(RankBatches& rb, const std::string& who, bpm_sampler* src, const RkWindow& w, bool folded, const double* d_arg, const int64_t* pos,
                            double* order_stats, Consume&& consume) {
    const uint32_t S = rb.S, dim = rb.dim, bc = rb.bc;
    const int32_t n_pos = rb.n_pos;
    std::vector<unsigned long long> hpos((size_t)n_pos);
    for (int32_t j = 0; j < n_pos; ++j) hpos[(size_t)j] = (unsigned long long)pos[j];
    if (n_pos > 0) HIPCK(hipMemcpyAsync(rb.d_pos.p, hpos.data(), hpos.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, src->stream));
    unsigned long long* k_in = rb.keys.p;
    unsigned long long* k_out = rb.keys.p + (size_t)bc * S;
    for (uint32_t k0 = 0; k0 < dim; k0 += bc) {
        const uint32_t b = std::min(bc, dim - k0);
        const uint32_t kw = std::min<uint32_t>(b, RK_THREADS), n_tiles = (b + kw - 1) / kw;
        uint64_t nby = 1;
        CK(rows_grid(w.S, n_tiles, (uint64_t)(RK_THREADS / kw) * RK_UNR, who.c_str(), &nby));
        hipLaunchKernelGGL(rk_keys_kernel, dim3(n_tiles, (unsigned)nby), dim3(RK_THREADS), 0, src->stream, (const double*)src->hist, src->ld, w, k0, b, kw,
                           folded ? 1u : 0u, d_arg, k_in);
        HIPCK(hipGetLastError());
        size_t t = rb.tmp_bytes;      // (the temporaries of a full batch hold those of the last, partial one)
        HIPCK(rank_sort(rb.tmp.p, &t, k_in, k_out, b, S, src->stream));
        if (n_pos > 0) {
            hipLaunchKernelGGL(rk_pick_kernel, dim3(((unsigned)n_pos * b + RK_THREADS - 1) / RK_THREADS), dim3(RK_THREADS), 0, src->stream,
                               (const unsigned long long*)k_out, w.S, k0, b, dim, (const unsigned long long*)rb.d_pos.p, (uint32_t)n_pos, rb.d_os.p);
            HIPCK(hipGetLastError());
        }
        CK(consume(k0, b, kw, n_tiles, nby, (const unsigned long long*)k_out));
    }
    if (n_pos > 0) HIPCK(hipMemcpyAsync(order_stats, rb.d_os.p, (size_t)n_pos * dim * sizeof(double), hipMemcpyDeviceToHost, src->stream));
    return 0;
}

// A RANKED HISTORY IS A HISTORY: a transform of the split rows of src's history rows [g_lo, g_hi) -- n = (g_hi - g_lo) / 2 rows from g_lo,
// then n rows up to g_hi -- written into the history of `dst`, a second, ordinary handle as bpm_derive_history takes one, with src's dim.
// kind RK_RANK: the average rank of a value among the S = 2 n n_local values of its coordinate; RK_Z: its normal score; RK_RANK_FOLDED,
// RK_Z_FOLDED: the same of |x - arg[k]|; RK_INDICATOR: x <= arg[k]; RK_SQDEV: (x - arg[k])^2 (the flat fills: no sort).  order_stats[j * dim + k] (sorted kinds): the pos[j]-th smallest value.  dst
// comes out as bpm_set_history leaves a handle and may be filled again.  Every check and every allocation of scratch comes before any
// launch; nothing src's sampler reads is written.
extern "C" int bpm_rank_history(bpm_handle_t src, bpm_handle_t dst, int64_t g_lo, int64_t g_hi, int32_t kind, const double* arg, int32_t n_pos,
                                const int64_t* pos, double* order_stats) {
    const std::string who = "bpm_rank_history";
    CK(second_handle_pair(who, src, dst, "the same dim"));
    if (kind < RK_RANK || kind > RK_SQDEV)
        return fail(who + ": kind must be 0 (rank), 1 (z), 2 (folded z), 3 (indicator), 4 (folded rank) or 5 (squared deviation); got " + std::to_string(kind));
    const bool flat = kind == RK_INDICATOR || kind == RK_SQDEV, sorted = !flat;
    if ((rk_folded(kind) || flat) && !arg) return fail(who + ": kind " + std::to_string(kind) + " needs arg (one value per coordinate)");
    if (n_pos < 0 || (n_pos > 0 && (!pos || !order_stats))) return fail(who + ": bad order-statistics arguments");
    if (kind == RK_INDICATOR && n_pos != 0) return fail(who + ": the indicator sorts nothing and has no order statistics (n_pos must be 0)");
    if (kind == RK_SQDEV && n_pos != 0) return fail(who + ": the squared deviation sorts nothing and has no order statistics (n_pos must be 0)");
    CK(require_resident_history(src, who.c_str()));
    CK(second_handle_single_rank(who, src, dst));
    if (g_lo < 0 || g_hi < g_lo || g_hi > src->hist_rows) return fail(who + ": generation range out of bounds");
    const int64_t n = (g_hi - g_lo) / 2;
    if (n < 4)
        return fail(who + ": a window of " + std::to_string((long long)(g_hi - g_lo)) + " history rows gives half-chains of " + std::to_string((long long)n) +
                    " draws; at least 4 are needed");
    CK(second_handle_fits(who, src, dst, src->dim, "the source has"));
    const uint64_t S64 = 2ull * (uint64_t)n * src->n_local;
    CK(rank_window_checks(who, S64, "ranked", n_pos, pos));
    const uint32_t S = (uint32_t)S64, dim = src->dim, ld = src->ld;
    size_t mem_free = 0, mem_total = 0;
    HIPCK(hipMemGetInfo(&mem_free, &mem_total));
    const int64_t rows = 2 * n;
    uint64_t hist_need = 0;
    CK(history_growth_bytes(dst, rows, who, "ranked", mem_free, &hist_need));
    mem_free -= (size_t)hist_need;      // (the scratch budget is what ensure_history will leave)
    RankBatches rb;
    DevTemp<double> d_arg;
    if (sorted) CK(rank_batches_plan(rb, who, src, S, mem_free, n_pos));
    if (rk_folded(kind) || flat) CK(d_arg.alloc(dim));
    // ---- nothing was launched so far ----
    CK(normalize_history(src, g_lo, g_hi));
    CK(ensure_history(dst, rows));
    if (d_arg.p) HIPCK(hipMemcpyAsync(d_arg.p, arg, (size_t)dim * sizeof(double), hipMemcpyHostToDevice, src->stream));
    RkWindow w;
    w.g_lo = (uint64_t)g_lo; w.g_up = (uint64_t)(g_hi - n); w.n = (uint64_t)n; w.n_local = src->n_local; w.S = S64; w.e0 = 0;
    if (!sorted) {
        const uint64_t total = S64 * ld;
        const unsigned nb = (unsigned)std::min<uint64_t>(2048, (total + RK_THREADS - 1) / RK_THREADS);
        hipLaunchKernelGGL(rk_indicator_kernel, dim3(nb), dim3(RK_THREADS), 0, src->stream, (const double*)src->hist, ld, dim, w, kind, (const double*)d_arg.p,
                           dst->hist);
        HIPCK(hipGetLastError());
    } else {
        CK(rank_batches_run(rb, who, src, w, rk_folded(kind), (const double*)d_arg.p, pos, order_stats,
                            [&](uint32_t k0, uint32_t b, uint32_t kw, uint32_t n_tiles, uint64_t nby, const unsigned long long* k_sorted) -> int {
                                hipLaunchKernelGGL(rk_score_kernel, dim3(n_tiles, (unsigned)nby), dim3(RK_THREADS), 0, src->stream, (const double*)src->hist, ld,
                                                   dim, w, k0, b, kw, kind, (const double*)d_arg.p, k_sorted, dst->hist);
                                HIPCK(hipGetLastError());
                                return 0;
                            }));
    }
    // the ln-likes of the same generations, and what bpm_set_history + bpm_set_loglike leave behind: the state = the last row, its ln-likes
    const size_t half = (size_t)n * src->n_local, row_d = (size_t)dst->n_local * dst->ld;
    HIPCK(hipMemcpyAsync(dst->llhist, src->llhist + (size_t)g_lo * src->n_local, half * sizeof(double), hipMemcpyDeviceToDevice, src->stream));
    HIPCK(hipMemcpyAsync(dst->llhist + half, src->llhist + (size_t)(g_hi - n) * src->n_local, half * sizeof(double), hipMemcpyDeviceToDevice, src->stream));
    HIPCK(hipMemcpyAsync(dst->G, dst->hist + (size_t)(rows - 1) * row_d, row_d * sizeof(double), hipMemcpyDeviceToDevice, src->stream));
    HIPCK(hipMemcpyAsync(dst->ll, src->llhist + (size_t)(g_hi - 1) * src->n_local, (size_t)dst->n_local * sizeof(double), hipMemcpyDeviceToDevice, src->stream));
    history_installed(dst, rows);
    HIPCK(hipStreamSynchronize(src->stream));
    return 0;
}

// THE HIGHEST-DENSITY INTERVAL of every coordinate over one window of s's history: per probability p, with m = min(floor(p S), S - 1) and the
// window's S values sorted, the first i of [0, S - m) whose width sorted[i + m] - sorted[i] is NaN (inf - inf) if one is, else the first of
// the smallest width, gives lo = sorted[i], hi = sorted[i + m] (ranks.h: rk_hdi_kernel over bpm_rank_history's sorted batches).  window 0:
// the split rows of history rows [a, b), bpm_rank_history's; window 1: the super-chain rows >= a (b is not read), bpm_reduce_moments'
// selection.  Every check and every allocation comes before any launch; s's history is only read, in chain order.
extern "C" int bpm_hdi(bpm_handle_t s, int32_t window, int64_t a, int64_t b, int32_t n_prob, const double* prob, int32_t n_pos, const int64_t* pos,
                       double* lo, double* hi, int64_t* n_nan, double* order_stats, int64_t* count) {
    const std::string who = "bpm_hdi";
    if (!s) return fail(who + ": null handle");
    CK(check_handle(s));
    CK(set_device(s));
    if (!lo || !hi || !n_nan || !count) return fail(who + ": null argument");
    if (window != 0 && window != 1) return fail(who + ": window must be 0 (the split rows of history rows [a, b)) or 1 (the super-chain rows >= a); got " + std::to_string(window));
    if (n_prob < 1 || n_prob > RK_MAX_PROB)
        return fail(who + ": n_prob = " + std::to_string(n_prob) + " is outside the supported 1 ... " + std::to_string(RK_MAX_PROB) + " probabilities per call");
    if (!prob) return fail(who + ": null argument (prob)");
    for (int32_t j = 0; j < n_prob; ++j)
        if (!(prob[j] > 0.0 && prob[j] < 1.0)) return fail(who + ": probability " + std::to_string(prob[j]) + " is outside (0, 1)");
    if (n_pos < 0 || (n_pos > 0 && (!pos || !order_stats))) return fail(who + ": bad order-statistics arguments");
    CK(require_resident_history(s, who.c_str()));
    if (s->world != 1) return fail(who + ": single rank only (world_size " + std::to_string(s->world) + ")");
    RkWindow w;
    int64_t r0 = 0, r1 = 0;      // the history rows the window reads
    if (window == 0) {
        if (a < 0 || b < a || b > s->hist_rows) return fail(who + ": generation range out of bounds");
        const int64_t n = (b - a) / 2;
        if (n < 1) return fail(who + ": the window is empty (" + std::to_string((long long)(b - a)) + " history rows give half-chains of no draws)");
        w.g_lo = (uint64_t)a; w.g_up = (uint64_t)(b - n); w.n = (uint64_t)n; w.n_local = s->n_local; w.S = 2ull * (uint64_t)n * s->n_local; w.e0 = 0;
        r0 = a; r1 = b;
    } else {
        uint64_t e_lo = 0, e_hi = 0;
        int64_t partial_row = -1;
        super_chain_bounds(s, a, &e_lo, &e_hi, &partial_row);
        if (e_hi <= e_lo) return fail(who + ": the window is empty (n_burn = " + std::to_string((long long)a) + " is at or beyond the last super-chain row)");
        w.g_lo = 0; w.g_up = 0; w.n = (uint64_t)s->hist_rows; w.n_local = s->n_local; w.S = e_hi - e_lo; w.e0 = e_lo;
        r0 = (int64_t)(e_lo / s->n_local); r1 = s->hist_rows;
    }
    CK(rank_window_checks(who, w.S, "sorted", n_pos, pos));
    const uint32_t S = (uint32_t)w.S, dim = s->dim;
    RkHdiOffsets off;
    for (int32_t j = 0; j < RK_MAX_PROB; ++j) off.m[j] = 0;
    for (int32_t j = 0; j < n_prob; ++j) off.m[j] = std::min<uint64_t>((uint64_t)std::floor(prob[j] * (double)S), (uint64_t)S - 1u);
    size_t mem_free = 0, mem_total = 0;
    HIPCK(hipMemGetInfo(&mem_free, &mem_total));
    RankBatches rb;
    CK(rank_batches_plan(rb, who, s, S, mem_free, n_pos));
    uint64_t parts = 1;
    CK(rows_grid(w.S, (uint64_t)rb.bc * (uint64_t)n_prob, (uint64_t)RK_THREADS * RK_UNR, who.c_str(), &parts));
    DevTemp<double> part_w, d_lo, d_hi;
    DevTemp<unsigned long long> part_i;
    DevTemp<long long> d_nan;
    const size_t n_part = (size_t)n_prob * rb.bc * (size_t)parts, n_res = (size_t)n_prob * dim;
    CK(part_w.alloc(n_part));
    CK(part_i.alloc(n_part));
    CK(d_lo.alloc(n_res));
    CK(d_hi.alloc(n_res));
    CK(d_nan.alloc(dim));
    // ---- nothing was launched so far ----
    CK(normalize_history(s, r0, r1));
    CK(rank_batches_run(rb, who, s, w, false, (const double*)nullptr, pos, order_stats,
                        [&](uint32_t k0, uint32_t bw, uint32_t, uint32_t, uint64_t, const unsigned long long* k_sorted) -> int {
                            hipLaunchKernelGGL(rk_hdi_kernel, dim3(bw, (unsigned)parts, (unsigned)n_prob), dim3(RK_THREADS), 0, s->stream, k_sorted, w.S, bw, off,
                                               part_w.p, part_i.p);
                            HIPCK(hipGetLastError());
                            hipLaunchKernelGGL(rk_hdi_final_kernel, dim3(((unsigned)n_prob * bw + RK_THREADS - 1) / RK_THREADS), dim3(RK_THREADS), 0, s->stream,
                                               k_sorted, w.S, k0, bw, dim, (uint32_t)n_prob, (uint32_t)parts, off, (const double*)part_w.p,
                                               (const unsigned long long*)part_i.p, d_lo.p, d_hi.p, d_nan.p);
                            HIPCK(hipGetLastError());
                            return 0;
                        }));
    static_assert(sizeof(long long) == sizeof(int64_t), "n_nan is copied as it lies");
    HIPCK(hipMemcpyAsync(lo, d_lo.p, n_res * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(hi, d_hi.p, n_res * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(n_nan, d_nan.p, (size_t)dim * sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    *count = (int64_t)w.S;
    return 0;
}

// the caller-owned-buffer form of rounds 1-4, compacted to the active work items.  Since round 5 the read-back runs in pieces INSIDE the call: the
// compaction copy of piece k (one host core reading freshly DMA'd memory: ~100 us for cfg2's 3.3 MB) runs under the DMA of piece k + 1 (~130 us); four
// pieces from 1 MB per half generation.
extern "C" int bpm_propose(bpm_handle_t s, double* out_prop, int32_t* out_ids, int32_t* n_out) {
    CK(check_handle(s));
    if (!out_prop || !out_ids || !n_out) return fail("bpm_propose: null argument");
    if (s->proposed) return fail("bpm_propose: previous proposals not committed");
    const size_t bytes = (size_t)(s->n_local / 2u + 1u) * s->ld * sizeof(double);
    static const int forced = getenv("BPM_PROPOSE_PIECES") ? atoi(getenv("BPM_PROPOSE_PIECES")) : 0;      // (A/B switch: tools/host_callback_ab.py)
    const int32_t pieces = forced > 0 ? std::min(forced, 256) : (bytes >= ((size_t)1 << 20) ? 4 : 1);
    // (cfg2's shape, 3.3 MB per half generation, two runs each: 1 piece 6.5 / 6.5e6 chain-updates/s, 2 pieces 6.9 / 5.7, 4 pieces 8.3 / 7.0, 8 pieces 5.7 / 5.5 --
    // every piece costs an event wait and a DMA submission: profiles/r05_host_callback.txt)
    CK(bpm_propose_begin(s, pieces));
    int32_t n = 0;
    for (int32_t k = 0; k < pieces; ++k) {
        const double* props = nullptr; const int32_t* ids = nullptr; int32_t nr = 0, ld = 0;
        CK(bpm_propose_chunk(s, k, &props, &ids, &nr, &ld));
        // compact the active work items (work-item order is kept; commit uses the same order)
        if (s->ld == s->dim && nr > 0) {                                  // (runs of active rows in one copy)
            int32_t w = 0;
            while (w < nr) {
                if (ids[w] < 0) { ++w; continue; }
                int32_t e = w;
                while (e < nr && ids[e] >= 0) ++e;
                std::memcpy(out_prop + (size_t)n * s->dim, props + (size_t)w * s->ld, (size_t)(e - w) * s->dim * sizeof(double));
                std::memcpy(out_ids + n, ids + w, (size_t)(e - w) * sizeof(int32_t));
                n += e - w; w = e;
            }
        } else {
            for (int32_t w = 0; w < nr; ++w) {
                if (ids[w] < 0) continue;
                std::memcpy(out_prop + (size_t)n * s->dim, props + (size_t)w * s->ld, s->dim * sizeof(double));
                out_ids[n++] = ids[w];
            }
        }
    }
    *n_out = n;
    s->prop_whole = true;
    return 0;
}

extern "C" int bpm_commit(bpm_handle_t s, const double* ll_prop) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->proposed) return fail("bpm_commit: nothing proposed");
    if (s->prop_mode != 1 || !s->prop_whole) return fail("bpm_commit: the open half generation was proposed with another entry point (bpm_propose_begin / bpm_propose_device)");
    const PhaseArgs& a = s->cur_args[s->phase];
    // scatter the values back to work-item order (the ids are still in the pinned buffer bpm_propose filled)
    std::vector<double> full(a.n_items, 0.0);
    size_t n = 0;
    for (uint32_t w = 0; w < a.n_items; ++w) {
        if (s->h_ids[w] < 0) continue;
        if (!ll_prop) return fail("bpm_commit: null ll_prop");
        full[w] = ll_prop[n++];
    }
    for (int32_t k = 0; k < s->prop_chunks; ++k) CK(bpm_commit_chunk(s, k, full.data() + chunk_lo(a.n_items, s->prop_chunks, k)));
    return bpm_commit_end(s);
}

// ---- the likelihood evaluated ON THE DEVICE by the caller's own framework (torch, cupy ...): nothing crosses PCIe --------------------------
extern "C" int bpm_propose_device(bpm_handle_t s, const double** rows_dev, const int32_t** ids_dev, int32_t* n_rows, int32_t* ld) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!rows_dev || !ids_dev || !n_rows || !ld) return fail("bpm_propose_device: null argument");
    CK(propose_launch(s, "bpm_propose_device"));
    const PhaseArgs& a = s->cur_args[s->phase];
    // (the active-row count for the accept bookkeeping: the ids come back, 32 KB; with one rank every work item is active)
    HIPCK(hipMemcpyAsync(s->h_ids, s->ids_buf, s->n_local * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));                  // the proposals are complete: the caller's framework reads them on ITS stream
    int64_t act = 0;
    for (uint32_t w = 0; w < a.n_items; ++w) act += s->h_ids[w] >= 0 ? 1 : 0;
    s->prop_active = act;
    *rows_dev = s->prop_buf; *ids_dev = s->ids_buf; *n_rows = (int32_t)a.n_items; *ld = (int32_t)s->ld;
    s->prop_mode = 2; s->prop_chunks = 0;
    s->proposed = true;
    return 0;
}

extern "C" int bpm_commit_device(bpm_handle_t s, const double* ll_dev) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->proposed || s->prop_mode != 2) return fail("bpm_commit_device: nothing proposed with bpm_propose_device");
    const PhaseArgs& a = s->cur_args[s->phase];
    if (a.n_items > 0) {
        if (!ll_dev) return fail("bpm_commit_device: null ll_dev");
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, ll_dev) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != s->cfg.device) {
            (void)hipGetLastError();
            return fail("bpm_commit_device: ll_dev must be device memory of this sampler's GPU (float64, one value per proposal row, contiguous)");
        }
        // the caller's framework may have computed the values on any stream of this device: wait for the device, then copy on ours
        HIPCK(hipDeviceSynchronize());
        HIPCK(hipMemcpyAsync(s->aux_buf + s->n_local, ll_dev, (size_t)a.n_items * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    }
    return commit_finish(s, s->prop_active);
}

// the local chains' CURRENT states where they lie in device memory (n_local rows of *ld doubles), and their ln-likes from device memory: what a
// device-resident likelihood needs once per (re)initialisation (the host form: bpm_get_state + bpm_set_loglike)
extern "C" int bpm_state_device(bpm_handle_t s, const double** rows_dev, int32_t* n_rows, int32_t* ld) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!rows_dev || !n_rows || !ld) return fail("bpm_state_device: null argument");
    HIPCK(hipStreamSynchronize(s->stream));
    *rows_dev = s->G + (uint64_t)s->rank * s->L.blk; *n_rows = (int32_t)s->n_local; *ld = (int32_t)s->ld;
    return 0;
}
extern "C" int bpm_set_loglike_device(bpm_handle_t s, const double* ll_dev) {
    CK(check_handle(s));
    CK(set_device(s));
    if (s->cfg.target_id != BPM_TARGET_HOST_CALLBACK) return fail("bpm_set_loglike_device: host-callback targets only");
    hipPointerAttribute_t at;
    if (!ll_dev || hipPointerGetAttributes(&at, ll_dev) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != s->cfg.device) {
        (void)hipGetLastError();
        return fail("bpm_set_loglike_device: ll_dev must be device memory of this sampler's GPU (float64, n_local values)");
    }
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemcpyAsync(s->ll, ll_dev, s->n_local * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (last_row_is_state(s))
        HIPCK(hipMemcpyAsync(s->llhist + (size_t)(s->hist_rows - 1) * s->n_local, s->ll, s->n_local * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int bpm_reserve_history(bpm_handle_t s, int64_t total_rows) {
    CK(check_handle(s));
    CK(set_device(s));
    return reserve_history(s, total_rows, "bpm_reserve_history");
}

// ---- thinned histories (chain.py:51-54 appends every generation; here every hist_stride-th) -------------------------------------------------
// what a stride above 1 cannot go with, by reason
static int check_history_stride(const bpm_sampler* s, const char* who, int64_t k) {
    if (k < 1) return fail(std::string(who) + ": the stride must be at least 1 (1 = a row per generation)");
    if (k > 1 && !s->cfg.keep_history) return fail(std::string(who) + ": this sampler keeps no history (keep_history=0): there is nothing to thin");
    if (k > 2147483647LL) return fail(std::string(who) + ": the stride would exceed 2^31 - 1");
    if (k > 1 && s->cfg.running_moments)
        return fail(std::string(who) + ": running_moments counts every generation, a thinned history every k-th: the two n_burn units would disagree; use one or the other");
    if (k > 1 && s->cfg.outlier_every > 0)
        return fail(std::string(who) + ": the outlier check (outlier_every > 0) reads a history row per generation; it cannot run on a thinned history");
    return 0;
}

extern "C" int bpm_set_history_thin(bpm_handle_t s, int32_t k) {
    CK(check_handle(s));
    CK(check_history_stride(s, "bpm_set_history_thin", k));
    if (k == s->hist_stride) return 0;
    if (s->rows_logical > 1 || s->hist_rows > 1)
        return fail("bpm_set_history_thin: the history already holds generations at stride " + std::to_string((long long)s->hist_stride) +
                    "; bpm_thin_history(h, m) thins what is stored (the new stride is a multiple of the old one)");
    s->hist_stride = k;
    return 0;
}

extern "C" int bpm_get_history_thin(bpm_handle_t s, int64_t out[4]) {
    CK(check_handle(s));
    if (!out) return fail("bpm_get_history_thin: null argument");
    out[0] = s->hist_stride;
    out[1] = s->rows_logical;
    out[2] = s->hist_rows;
    out[3] = s->hist_rows >= 1 ? (s->hist_rows - 1) * s->hist_stride : -1;
    return 0;
}

// Keep stored rows 0, m, 2m, ... : gathered into buffers of exactly that many rows (hist_thin_kernel, on the HIP stream), which then take the old
// ones' place in the registry as ensure_history's do; the old memory goes back.  Reads and writes new rows x n_local x (ld + 1) x 8 bytes once.
extern "C" int bpm_thin_history(bpm_handle_t s, int32_t m) {
    const char* who = "bpm_thin_history";
    CK(check_handle(s));      // (leave_direct: kernels in flight on the library's own queue still write the old buffers)
    CK(set_device(s));
    if (m < 1) return fail(std::string(who) + ": m must be at least 1 (1 = keep every stored row)");
    if (m == 1) return 0;
    CK(check_history_stride(s, who, s->hist_stride * (int64_t)m));
    if (!history_resident(s) || s->hist_rows < 1) return fail(std::string(who) + ": no resident history (initialise the chains first)");
    if (s->proposed || s->phase != 0) return fail(std::string(who) + ": a generation is open (bpm_propose without its bpm_commit); finish it first");
    const int64_t rows_new = (s->hist_rows - 1) / m + 1;
    const size_t row_d = (size_t)s->n_local * s->ld;
    DevTemp<double> nh, nl;
    CK(nh.alloc((size_t)rows_new * row_d, who, "the thinned history's " + std::to_string((long long)rows_new) + " rows"));
    CK(nl.alloc((size_t)rows_new * s->n_local));
    const unsigned gy = (unsigned)std::min<int64_t>(rows_new, 65535);
    const uint64_t tile = (uint64_t)THIN_THREADS * THIN_UNR;
    {   // state rows: ld is even, every row starts on 16 bytes
        const uint64_t row_v = row_d / 2u;
        hipLaunchKernelGGL(hist_thin_kernel<double2>, dim3((unsigned)((row_v + tile - 1) / tile), gy), dim3(THIN_THREADS), 0, s->stream,
                           reinterpret_cast<const double2*>(s->hist), reinterpret_cast<double2*>(nh.p), row_v, (uint64_t)rows_new, (uint64_t)m);
    }
    if (s->n_local % 2u == 0u) {
        const uint64_t row_v = s->n_local / 2u;
        hipLaunchKernelGGL(hist_thin_kernel<double2>, dim3((unsigned)((row_v + tile - 1) / tile), gy), dim3(THIN_THREADS), 0, s->stream,
                           reinterpret_cast<const double2*>(s->llhist), reinterpret_cast<double2*>(nl.p), row_v, (uint64_t)rows_new, (uint64_t)m);
    } else {      // an odd number of ln-likes per row: every other row starts 8 bytes off
        const uint64_t row_v = s->n_local;
        hipLaunchKernelGGL(hist_thin_kernel<double>, dim3((unsigned)((row_v + tile - 1) / tile), gy), dim3(THIN_THREADS), 0, s->stream,
                           (const double*)s->llhist, nl.p, row_v, (uint64_t)rows_new, (uint64_t)m);
    }
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(s->stream));
    // (nothing of the sampler has changed up to here; nothing below can fail)
    s->mem.replace(&s->hist, nh);
    s->mem.replace(&s->llhist, nl);
    s->hist_cap = rows_new;
    for (int64_t r = 0; r < rows_new; ++r) s->hist_tag[(size_t)r] = s->hist_tag[(size_t)(r * m)];      // a row kept in position order moves with its tag
    s->hist_tag.resize((size_t)rows_new, -1);
    s->hist_rows = rows_new;
    s->hist_stride *= m;
    s->hist_epoch += 1;
    return 0;
}

extern "C" int bpm_set_history_thinned(bpm_handle_t s, int64_t rows, const double* hist_local, const double* X, int32_t k, int64_t rows_logical) {
    const char* who = "bpm_set_history_thinned";
    CK(check_handle(s));
    if (rows < 1 || !hist_local || !X) return fail(std::string(who) + ": bad argument");
    CK(check_history_stride(s, who, k));
    if (rows_logical < 1 || rows != (rows_logical - 1) / k + 1)
        return fail(std::string(who) + ": " + std::to_string((long long)rows) + " stored rows do not agree with " + std::to_string((long long)rows_logical) +
                    " logical rows at stride " + std::to_string(k) + " (rows must be (rows_logical - 1) / k + 1)");
    // (X is the last stored row only when the last generation was stored: otherwise every row comes from hist_local, a single one too)
    const int64_t stride_was = s->hist_stride;
    if (install_history(s, who, rows, hist_local, X, (rows_logical - 1) % k == 0) != 0) {
        s->hist_stride = stride_was;      // (an error in there leaves the handle as a failed bpm_set_history does -- re-initialised at X -- with its stride)
        return 1;
    }
    s->hist_stride = k;
    s->rows_logical = rows_logical;
    s->w_rows = 0;      // (moments are rebuilt from the stored rows when adaptation next needs them)
    return 0;
}

#ifdef BPM_TEST_HOOKS
// Test variant only: the Welford records of this rank's chains, mean and m2 as n_local x ld each
extern "C" int bpm_debug_get_welford(bpm_handle_t s, double* mean, double* m2) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!mean || !m2) return fail("bpm_debug_get_welford: null argument");
    const size_t w = (size_t)s->ld * sizeof(double);
    HIPCK(hipMemcpy2DAsync(mean, w, s->w_mean, 2 * w, w, s->n_local, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpy2DAsync(m2, w, s->w_m2, 2 * w, w, s->n_local, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}
#endif   // BPM_TEST_HOOKS

// Large device-to-host transfers into the caller's pageable buffer.  HIP's own pageable path stages through pinned
// memory with ONE host thread copying out of it (~10 GB/s here, and the caller's fresh NumPy array page-faults on
// first touch on that same thread).  Here `n_workers` host threads, each with its own stream and two pinned staging
// buffers, take chunks from a shared counter: the DMA of a thread's next chunk overlaps its memcpy of the current one.
static int d2h_rows_parallel(bpm_sampler* s, double* out, const double* src, size_t rows, uint32_t dim, uint32_t ld) {
    const size_t row_bytes = (size_t)dim * sizeof(double);
    const size_t chunk_rows = std::max<size_t>(1, ((size_t)8 << 20) / row_bytes);
    const size_t n_chunks = (rows + chunk_rows - 1) / chunk_rows;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int n_workers = (int)std::min<size_t>(std::min<size_t>(8, std::max(1u, hw / 2)), n_chunks);
    {   // the caller's buffer is typically a fresh anonymous mapping (np.empty): ask for transparent huge pages before the
        // first touch -- 800 k page faults of 4 KiB otherwise cost as much as the copy itself
        const uintptr_t b0 = ((uintptr_t)out + 4095u) & ~(uintptr_t)4095u, b1 = ((uintptr_t)out + rows * row_bytes) & ~(uintptr_t)4095u;
        if (b1 > b0) (void)madvise((void*)b0, (size_t)(b1 - b0), MADV_HUGEPAGE);
    }
    std::atomic<size_t> next{0};
    std::atomic<int> err{0};
    const int device = s->cfg.device;
    auto work = [&]() {
        hipStream_t st = nullptr;
        DevTemp<double> pinned[2] = {DevTemp<double>(MEM_PINNED), DevTemp<double>(MEM_PINNED)};
        auto ok = [&](hipError_t e) { if (e != hipSuccess) { err.store((int)e); return false; } return true; };
        if (ok(hipSetDevice(device)) && ok(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) &&
            ok(pinned[0].get(chunk_rows * dim)) && ok(pinned[1].get(chunk_rows * dim))) {
            double* const pin[2] = {pinned[0].p, pinned[1].p};
            auto issue = [&](size_t ch, int b) {
                const size_t r0 = ch * chunk_rows, nr = std::min(chunk_rows, rows - r0);
                return ok(hipMemcpy2DAsync(pin[b], row_bytes, src + r0 * ld, (size_t)ld * sizeof(double), row_bytes, nr,
                                           hipMemcpyDeviceToHost, st));
            };
            size_t cur = next.fetch_add(1);
            int b = 0;
            bool live = cur < n_chunks && issue(cur, b);
            while (live && err.load() == 0) {
                if (!ok(hipStreamSynchronize(st))) break;                 // chunk `cur` is in pin[b]
                const size_t nxt = next.fetch_add(1);
                const bool more = nxt < n_chunks;
                if (more && !issue(nxt, b ^ 1)) break;                    // next DMA runs under this memcpy
                const size_t r0 = cur * chunk_rows, nr = std::min(chunk_rows, rows - r0);
                std::memcpy(out + r0 * dim, pin[b], nr * row_bytes);
                if (!more) break;
                cur = nxt;
                b ^= 1;
            }
            if (st) (void)hipStreamSynchronize(st);
        }
        if (st) (void)hipStreamDestroy(st);
    };
    std::vector<std::thread> th;
    for (int w = 1; w < n_workers; ++w) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    if (err.load() != 0) return fail(std::string("bpm_get_history: ") + hipGetErrorString((hipError_t)err.load()));
    return 0;
}

extern "C" int bpm_get_history(bpm_handle_t s, int64_t g_lo, int64_t g_hi, double* out) {
    CK(check_handle(s));
    CK(set_device(s));
    if (g_lo < 0 || g_hi < g_lo || g_hi > s->hist_rows) return fail("bpm_get_history: generation range out of bounds");
    if (g_hi == g_lo) return 0;
    if (!out) return fail("bpm_get_history: null argument");
    CK(normalize_history(s, g_lo, g_hi));
    const size_t rows = (size_t)(g_hi - g_lo) * s->n_local;
    if (rows * s->dim * sizeof(double) >= ((size_t)128 << 20)) {
        HIPCK(hipStreamSynchronize(s->stream));
        return d2h_rows_parallel(s, out, s->hist + (uint64_t)g_lo * s->n_local * s->ld, rows, s->dim, s->ld);
    }
    HIPCK(hipMemcpy2DAsync(out, s->dim * sizeof(double), s->hist + (uint64_t)g_lo * s->n_local * s->ld,
                           s->ld * sizeof(double), s->dim * sizeof(double), rows, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int bpm_get_loglike_history(bpm_handle_t s, int64_t g_lo, int64_t g_hi, double* out) {
    CK(check_handle(s));
    CK(set_device(s));
    if (g_lo < 0 || g_hi < g_lo || g_hi > s->hist_rows) return fail("bpm_get_loglike_history: range out of bounds");
    if (g_hi == g_lo) return 0;
    CK(normalize_history(s, g_lo, g_hi));
    HIPCK(hipMemcpyAsync(out, s->llhist + (uint64_t)g_lo * s->n_local, (size_t)(g_hi - g_lo) * s->n_local * sizeof(double),
                         hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int bpm_get_stats(bpm_handle_t s, bpm_stats_t* out) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!out) return fail("bpm_get_stats: null argument");
    unsigned long long c[8];
    double cr[3 * MAX_CR];
    std::vector<uint32_t> acc((size_t)s->n_local + ACC_SHARDS);       // per-chain counters and per-wavefront shards: the total is what counts
    HIPCK(hipMemcpyAsync(c, s->counters, sizeof(c), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(cr, s->cr_state, sizeof(cr), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(acc.data(), s->acc_count, acc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    std::memset(out, 0, sizeof(*out));
    int64_t n_acc = 0;
    for (uint32_t v : acc) n_acc += v;
    // every local chain is updated exactly once per generation (it is in exactly one of the two pools)
    const int64_t n_upd = s->k_gen * (int64_t)s->n_local + (s->phase == 1 ? s->phase_a_updates : 0);
    out->local_n_accepted = n_acc;                       // demc.py:67,190
    out->local_n_rejected = 1 + n_upd - n_acc;           // demc.py:68,193: starts at 1
    out->n_nan_alpha = (int64_t)c[2];
    out->k_gen = s->k_gen;
    out->t_abs = s->t_abs;
    out->history_rows = s->hist_rows;
    out->n_outlier_resets = (int64_t)c[4];
    out->n_cr = s->cfg.n_cr;
    for (int m = 0; m < MAX_CR; ++m) {
        out->p_cr[m] = cr[m];
        out->delta_m[m] = cr[MAX_CR + m];
        out->n_cr_updates[m] = cr[2 * MAX_CR + m];
    }
    return 0;
}

extern "C" int bpm_set_adapt_state(bpm_handle_t s, const double* p_cr, const double* delta_m, const double* n_cr_updates,
                                   int64_t t_abs) {
    CK(check_handle(s));
    CK(set_device(s));
    double cr[3 * MAX_CR] = {0};
    for (int m = 0; m < s->cfg.n_cr; ++m) {
        cr[m] = p_cr ? p_cr[m] : 1.0 / s->cfg.n_cr;
        cr[MAX_CR + m] = delta_m ? delta_m[m] : 0.0;
        cr[2 * MAX_CR + m] = n_cr_updates ? n_cr_updates[m] : 0.0;
    }
    HIPCK(hipMemcpyAsync(s->cr_state, cr, sizeof(cr), hipMemcpyHostToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    if (t_abs >= 0) s->t_abs = t_abs;
    return 0;
}

extern "C" int bpm_eval_loglike(bpm_handle_t s, const double* X, int32_t n, double* out) {
    CK(check_handle(s));
    CK(set_device(s));
    if (n <= 0) return 0;
    if (!X || !out) return fail("bpm_eval_loglike: null argument");
    DevTemp<double> bX, bO;
    CK(bX.alloc((size_t)n * s->ld));
    CK(bO.alloc((size_t)n));
    double* const dX = bX.p;
    double* const dO = bO.p;
    HIPCK(hipMemsetAsync(dX, 0, (size_t)n * s->ld * sizeof(double), s->stream));
    HIPCK(hipMemcpy2DAsync(dX, s->ld * sizeof(double), X, s->dim * sizeof(double), s->dim * sizeof(double), n,
                           hipMemcpyHostToDevice, s->stream));
    if (!launch_eval_target(s, dX, (uint32_t)n, dO)) return fail("bpm_eval_loglike: host-callback target has no device ln_like");
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(out, dO, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return 0;
}

#ifdef BPM_TEST_HOOKS
// ---- debug / parity hooks (include/bipymc_hip_test.h; build_variants/libbipymc_test.so only) ------------------------------------------
extern "C" int bpm_set_trace(bpm_handle_t s, int32_t on) {
    CK(check_handle(s));
    CK(set_device(s));
    HIPCK(hipStreamSynchronize(s->stream));
    if (on && !s->trace_i32) {
        CK(s->mem.alloc(&s->trace_i32, (size_t)s->n_local * TRACE_I32));
        CK(s->mem.alloc(&s->trace_f64, (size_t)s->n_local * TRACE_F64));
        CK(s->mem.alloc(&s->trace_mask, (size_t)s->n_local * s->dim));
        HIPCK(hipMemset(s->trace_i32, 0xFF, (size_t)s->n_local * TRACE_I32 * sizeof(int32_t)));
        HIPCK(hipMemset(s->trace_f64, 0, (size_t)s->n_local * TRACE_F64 * sizeof(double)));
        HIPCK(hipMemset(s->trace_mask, 0, (size_t)s->n_local * s->dim));
    } else if (!on && s->trace_i32) {
        s->mem.release(&s->trace_i32); s->mem.release(&s->trace_f64); s->mem.release(&s->trace_mask);
    }
    return 0;
}

// trace of the LAST generation: out_i32 [n_local*32] = (cr_idx, d_prime, jump, accepted, snooker, partners[23]..),
// out_f64 [n_local*4] = (alpha, ll_prop, delta, gamma), out_mask [n_local*dim]
extern "C" int bpm_get_trace(bpm_handle_t s, int32_t* out_i32, double* out_f64, uint8_t* out_mask) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->trace_i32) return fail("bpm_get_trace: tracing is off");
    HIPCK(hipStreamSynchronize(s->stream));
    if (out_i32) HIPCK(hipMemcpy(out_i32, s->trace_i32, (size_t)s->n_local * TRACE_I32 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_f64) HIPCK(hipMemcpy(out_f64, s->trace_f64, (size_t)s->n_local * TRACE_F64 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_mask) HIPCK(hipMemcpy(out_mask, s->trace_mask, (size_t)s->n_local * s->dim, hipMemcpyDeviceToHost));
    return 0;
}

// the host-side per-generation decisions, for parity against oracle/philox_ref.py
extern "C" int bpm_debug_perm(bpm_handle_t s, int64_t t, int32_t shuffle, double flip_prob, int32_t* out_order,
                              int32_t* out_inverse, int32_t* out_flip) {
    CK(check_handle(s));
    const PermKey pk = make_perm_key(s->cfg.seed, (uint64_t)t, s->N, shuffle != 0);
    for (uint32_t x = 0; x < s->N; ++x) {
        if (out_order) out_order[x] = (int32_t)perm_fwd(x, pk);
        if (out_inverse) out_inverse[x] = (int32_t)perm_inv(x, pk);
    }
    if (out_flip) *out_flip = flip_draw(s->cfg.seed, (uint64_t)t, flip_prob) ? 1 : 0;
    return 0;
}

extern "C" int bpm_selftest_philox(int32_t device, int32_t n, uint64_t seed, uint32_t* out_mine, uint32_t* out_rocrand) {
    if (n <= 0 || !out_mine || !out_rocrand) return fail("bpm_selftest_philox: bad argument");
    HIPCK(hipSetDevice(device));
    DevTemp<uint32_t> d;
    CK(d.alloc((size_t)n * 8));
    launch_rocrand_check(d.p, n, seed);
    HIPCK(hipGetLastError());
    HIPCK(hipDeviceSynchronize());
    std::vector<uint32_t> h((size_t)n * 8);
    HIPCK(hipMemcpy(h.data(), d.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        std::memcpy(out_mine + 4 * (size_t)i, h.data() + 8 * (size_t)i, 16);
        std::memcpy(out_rocrand + 4 * (size_t)i, h.data() + 8 * (size_t)i + 4, 16);
    }
    return 0;
}

// The accept test of the update kernels (accept_test.h) on n caller-supplied (d, u) pairs, evaluated on the device: its decision and NaN flag beside the
// plain formula's with the device library's exp(), and whether the float32 filter asked for the exact path.  One byte per case and array.
extern "C" int bpm_selftest_accept(int32_t device, int32_t n, const double* d, const double* u, uint8_t* accepted_filter, uint8_t* accepted_exact,
                                   uint8_t* nan_filter, uint8_t* nan_exact, uint8_t* took_exact) {
    if (n <= 0 || !d || !u || !accepted_filter || !accepted_exact || !nan_filter || !nan_exact || !took_exact) return fail("bpm_selftest_accept: bad argument");
    HIPCK(hipSetDevice(device));
    DevTemp<double> dd, du;
    DevTemp<uint8_t> dout;
    CK(dd.alloc((size_t)n)); CK(du.alloc((size_t)n)); CK(dout.alloc((size_t)n * 5));
    HIPCK(hipMemcpy(dd.p, d, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(du.p, u, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(accept_check_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, (int)n, dd.p, du.p, dout.p);
    HIPCK(hipGetLastError());
    HIPCK(hipDeviceSynchronize());
    std::vector<uint8_t> h((size_t)n * 5);
    HIPCK(hipMemcpy(h.data(), dout.p, h.size(), hipMemcpyDeviceToHost));
    uint8_t* const outs[5] = {accepted_filter, accepted_exact, nan_filter, nan_exact, took_exact};
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 5; ++k) outs[k][i] = h[5 * (size_t)i + k];
    return 0;
}

// The measured error of the accept test's float32 route: out[0] = max over EVERY float t in [-58, -2^-20] of |(double)exp2_f32(t) / exp2_f64(t) - 1| (one
// launch), out[1] = max over the n given d of |route(d) / exp(d) - 1| with the device library's exp.
extern "C" int bpm_selftest_accept_error(int32_t device, int32_t n, const double* d, double out[2]) {
    if (n <= 0 || !d || !out) return fail("bpm_selftest_accept_error: bad argument");
    HIPCK(hipSetDevice(device));
    DevTemp<double> dd;
    DevTemp<unsigned long long> slots;
    CK(dd.alloc((size_t)n)); CK(slots.alloc(2));
    HIPCK(hipMemcpy(dd.p, d, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCK(hipMemset(slots.p, 0, 2 * sizeof(unsigned long long)));
    const float t_small = 0x1p-20f, t_big = 58.0f;
    uint32_t b_lo, b_hi;
    std::memcpy(&b_lo, &t_small, 4); std::memcpy(&b_hi, &t_big, 4);
    hipLaunchKernelGGL(accept_exp2_sweep_kernel, dim3(4096), dim3(256), 0, 0, b_lo, b_hi, slots.p);
    hipLaunchKernelGGL(accept_route_kernel, dim3(1024), dim3(256), 0, 0, (int)n, dd.p, slots.p + 1);
    HIPCK(hipGetLastError());
    HIPCK(hipDeviceSynchronize());
    unsigned long long h[2];
    HIPCK(hipMemcpy(h, slots.p, sizeof(h), hipMemcpyDeviceToHost));
    std::memcpy(out, h, sizeof(h));
    return 0;
}

// Test hook: the quartile / best-chain selection of the outlier check on caller-supplied omega values (world_size 1, sampler created
// with outlier_every > 0): out = (sorted[k0], sorted[k0 + 1], sorted[k1], sorted[k1 + 1], first argmax, cut = Q1 - 2 IQR) with the
// order statistics np.percentile(omega, [25, 75]) interpolates between.  tests/test_gpu_parity.py compares with NumPy on ties,
// infinities, signed zeros and all-equal inputs.
extern "C" int bpm_debug_outlier_select(bpm_handle_t s, const double* omega, double out[6]) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!omega || !out) return fail("bpm_debug_outlier_select: null argument");
    if (!s->om || s->world != 1) return fail("bpm_debug_outlier_select: needs a single-rank sampler created with outlier_every > 0");
    const uint32_t N = s->N;
    HIPCK(hipMemcpyAsync(s->om, omega, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s->stream));
    SelRanks R;
    double tq[2];
    for (int i = 0; i < 2; ++i) {
        const double pos = (i == 0 ? 25.0 : 75.0) / 100.0 * (double)(N - 1);
        const uint32_t lo = (uint32_t)std::floor(pos);
        R.k[2 * i] = lo;
        R.k[2 * i + 1] = std::min(lo + 1u, N - 1u);
        tq[i] = pos - (double)lo;
    }
    launch_outlier_select(s, R);
    HIPCK(hipGetLastError());
    double h[5];
    HIPCK(hipMemcpyAsync(h, s->sel, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    for (int i = 0; i < 5; ++i) out[i] = h[i];
    auto lerp = [](double a, double b, double t) { const double d = b - a; return t >= 0.5 ? b - d * (1.0 - t) : a + d * t; };
    const double q1 = lerp(h[0], h[1], tq[0]), q3 = lerp(h[2], h[3], tq[1]);
    out[5] = q1 - 2.0 * (q3 - q1);
    return 0;
}

// Diagnostic (tools/emulate_ranks.py): the update kernel and the replay kernel of this handle's LAST half generation launched
// `reps` times back to back and timed with an event pair -- DESTRUCTIVE (the replica is advanced again and again), for timing
// only.  Why: R ranks emulated on one GPU share ONE Infinity Cache, so kernel times read from a trace of the lock-step run are
// those of a GPU whose cache holds eight replicas; re-launching one rank's kernels alone shows them with that rank's data warm.
extern "C" int bpm_debug_time_kernels(bpm_handle_t s, int32_t reps, float* update_us, float* replay_us) {
    CK(check_handle(s));
    CK(set_device(s));
    if (reps < 1 || !update_us || !replay_us) return fail("bpm_debug_time_kernels: bad argument");
    if (!pick_fused(s)) return fail("bpm_debug_time_kernels: device targets only");
    const PhaseArgs& a = s->cur_args[1];
    if (a.n_items == 0) return fail("bpm_debug_time_kernels: run at least one generation first");
    HIPCK(hipStreamSynchronize(s->stream));
    *update_us = 0.f; *replay_us = 0.f;
    for (int which = 0; which < 2; ++which) {
        if (which == 1 && (!s->accbits_all || s->world == 1 || a.accbits == nullptr)) break;     // no replay exchange on this handle
        PhaseArgs r = a;      // (the update launch itself is relaunched as prepare_generation laid it out: cur_args[1] with the flavour chosen for it)
        if (which == 1) {
            r.replay = 1u; r.accbits = nullptr; r.accbits_all = s->accbits_all;
            trace_set(r, nullptr, nullptr, nullptr); r.pack = nullptr; r.hist_row = nullptr; r.llhist_row = nullptr;
            r.adapt_on = 0u;
        }
        for (int i = 0; i < 3; ++i) { if (which == 0) launch_update(s, 1); else launch_replay_any(s, r); }
        HIPCK(hipEventRecord(s->ev0, s->stream));
        for (int i = 0; i < reps; ++i) { if (which == 0) launch_update(s, 1); else launch_replay_any(s, r); }
        HIPCK(hipEventRecord(s->ev1, s->stream));
        HIPCK(hipEventSynchronize(s->ev1));
        HIPCK(hipGetLastError());
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        (which == 0 ? *update_us : *replay_us) = ms * 1e3f / (float)reps;
    }
    return 0;
}

// Test hook: this handle's update launches so far by kernel flavour (kernels.h: Flavour)
extern "C" int bpm_debug_flavour_counts(bpm_handle_t s, int64_t out[7]) {
    CK(check_handle_keep_direct(s));
    if (!out) return fail("bpm_debug_flavour_counts: null argument");
    static_assert(N_FLAVOURS == 7, "bpm_debug_flavour_counts reports 7 counts");
    for (int f = 0; f < N_FLAVOURS; ++f) out[f] = s->n_by_flavour[f];
    return 0;
}

// Test hook: the argument block the host hands kernel `index` of those it dispatches by packets of its own -- the side kernels as launch_side lays
// them out (from the function-pointer types its callers pass), the update kernels as FusedKernarg's members.  (tests/test_abi.py holds them
// against the code object's own metadata, on a machine without a GPU.)
struct KernargRow { const char* name; size_t n; const size_t* off; const size_t* size; };
template <class... P>
static KernargRow kernarg_row(const char* name, void (*)(P...)) {
    static constexpr KernargLayout<P...> lay;
    static_assert(lay.n <= 8, "bpm_debug_kernarg_layout reports up to 8 arguments");
    return {name, lay.n, lay.off, lay.size};
}
static KernargRow fused_kernarg_row(const char* name) {
    static const size_t off[] = {offsetof(FusedKernarg, pl_plan), offsetof(FusedKernarg, pl_upd_off), offsetof(FusedKernarg, pl_n_items), offsetof(FusedKernarg, pl_mode), offsetof(FusedKernarg, a)};
    static const size_t size[] = {sizeof(FusedKernarg::pl_plan), sizeof(FusedKernarg::pl_upd_off), sizeof(FusedKernarg::pl_n_items), sizeof(FusedKernarg::pl_mode), sizeof(FusedKernarg::a)};
    return {name, 5, off, size};
}
extern "C" int bpm_debug_kernarg_layout(int32_t index, const char** name, int32_t* n_args, int64_t offsets[8], int64_t sizes[8]) {
#define ROW(k) kernarg_row(#k, k)
    static const KernargRow rows[] = {ROW(moments_partial_kernel), ROW(moments_final_kernel), ROW(perm_table_kernel), ROW(plan_kernel), kernarg_row("cr_final_kernel", cr_final_kernel<1>),
                                      kernarg_row("cr_level1_kernel", cr_level1_kernel<4>), ROW(cr_mid_kernel), ROW(push_sync_kernel), ROW(push_arena_probe_kernel),
                                      fused_kernarg_row("phase_fused_kernel"), fused_kernarg_row("phase_wide_kernel")};
#undef ROW
    if (index < 0 || index >= (int32_t)(sizeof(rows) / sizeof(rows[0]))) return fail("bpm_debug_kernarg_layout: no kernel of that index");
    const KernargRow& r = rows[index];
    *name = r.name; *n_args = (int32_t)r.n;
    for (size_t i = 0; i < r.n; ++i) { offsets[i] = (int64_t)r.off[i]; sizes[i] = (int64_t)r.size[i]; }
    return 0;
}

#endif   // BPM_TEST_HOOKS

#ifdef BPM_STAMPS
// diagnostic build only: per-work-item s_memtime stamps of the LAST launched phase kernel
extern "C" int bpm_debug_stamps(bpm_handle_t s, unsigned long long* out, int64_t n_items) {
    CK(check_handle(s));
    CK(set_device(s));
    if (!s->stamps) {
        CK(s->mem.alloc(&s->stamps, (size_t)s->n_local * 8));
        HIPCK(hipMemset(s->stamps, 0, (size_t)s->n_local * 8 * sizeof(unsigned long long)));
        return 0;
    }
    HIPCK(hipStreamSynchronize(s->stream));
    if (out) HIPCK(hipMemcpy(out, s->stamps, (size_t)n_items * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}
#endif
