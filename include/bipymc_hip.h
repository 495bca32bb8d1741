/*
 * bipymc_hip.h -- C ABI of the MI355X-native DE-MC / DREAM population sampler.
 *
 * This is the drop-in boundary for the per-generation hot path of
 * wgurecky/bipymc's parallel samplers (reference paths relative to
 * /root/reference):
 *
 *   DeMcMpi._mcmc_run            bipymc/demc.py:63-151   generation driver, a/b pools, 2x Allgather
 *   DeMcMpi._update_chain_pool   bipymc/demc.py:153-196  DE-MC proposal + Metropolis
 *   DreamMpi._update_chain_pool  bipymc/dream.py:32-107  DREAM proposal (CR mask, multi-pair jump, jitter)
 *   DreamMpi._update_cr_ratios   bipymc/dream.py:119-140 crossover-probability adaptation
 *   DeMc._mut_prop_ratio / metropolis_accept  bipymc/samplers.py:328-336
 *   var_ball / var_box           bipymc/util.py:5-28
 *   McmcChain history            bipymc/chain.py:13-29,51-54,122-124
 *   targets                      bipymc/utils/{d100_gauss,dblgauss_rv,banana_rv}.py
 *   param_est / _super_chain     bipymc/demc.py:235-270
 *
 * The reference is pure Python and has no FFI of its own; the binding a
 * maintainer would add is the ctypes stub in INTEGRATION.md (the host-side
 * classes in bipymc_amd/{demc,dream}.py are that stub, written out).
 *
 * Conventions: opaque handle; every call returns 0 on success, non-zero on
 * error, and bpm_last_error() returns the message of the calling thread's last
 * failure.  No exceptions cross the boundary.  All buffers are caller-owned
 * host memory, row-major float64 unless stated; the library copies.  One host
 * thread per handle.  With world_size > 1 every rank must make the same
 * sequence of collective calls (create, init/set_state, begin_run, step,
 * propose/commit), exactly as all MPI ranks of the reference enter
 * comm.Allgather / comm.Barrier in lock-step.
 */
#ifndef BIPYMC_HIP_H
#define BIPYMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: bpm_step_timed gained n_launches (round 2) and the entry points below it were added; a caller built against version 1 is
 * refused by bpm_create / by the binding's bpm_abi_version check instead of passing a short argument list. */
#define BPM_ABI_VERSION 2

/* algo */
#define BPM_ALGO_DEMC 0  /* bipymc/demc.py:153-196 */
#define BPM_ALGO_DREAM 1 /* bipymc/dream.py:32-107 */
#define BPM_ALGO_DEMC_SYNC 2 /* bipymc/samplers.py:237-308 serial DeMc with delayed_accept=True: all chains
                              propose against the generation's starting states, updates banked; no a/b pools */

/* target ids: which ln_like_fn is evaluated on the device */
#define BPM_TARGET_HOST_CALLBACK 0  /* arbitrary Python ln_like_fn (samplers.py:36-43): propose/commit */
#define BPM_TARGET_GAUSS_EQUICORR 1 /* utils/d100_gauss.py:14-35; params [rho,c0,a,b,1/sigma_0..d-1] */
#define BPM_TARGET_MIXTURE_PAIRS 2  /* utils/dblgauss_rv.py:11-32 (d=2) and its pairwise d-dim extension */
#define BPM_TARGET_BANANA_2D 3      /* utils/banana_rv.py:11-37 */

#define BPM_MAX_CR 8
#define BPM_UID_BYTES 128
#define BPM_PUSH_BLOB_BYTES 256

typedef struct bpm_sampler* bpm_handle_t;

/* Constructor arguments: DeMcMpi.__init__ (demc.py:14-32) / DreamMpi.__init__ (dream.py:17-30). */
typedef struct bpm_config {
    int32_t abi_version; /* BPM_ABI_VERSION */
    int32_t algo;        /* BPM_ALGO_* */
    int32_t n_chains;    /* global number of chains, >= 4 (samplers.py:249), divisible by world_size */
    int32_t dim;         /* len(theta_0) or kwargs["dim"] (demc.py:20-23); 1 ... 131055 and n_chains * (dim + 2) < 2^31 (the reference has no limit;
                          * rows wider than 512 coordinates run on the looped kernel, bipymc_amd/csrc/kernels_wide.h) */
    int32_t target_id;   /* BPM_TARGET_* */
    int32_t n_target_params;
    const double* target_params; /* copied */
    uint64_t seed;               /* np.random.seed(...) analogue: key of every Philox stream */
    int32_t device;              /* HIP device ordinal */
    int32_t rank;                /* comm.rank; owns chains array_split(range(N), size)[rank] (demc.py:39) */
    int32_t world_size;          /* comm.size */
    const char* nccl_uid;        /* BPM_UID_BYTES from bpm_get_unique_id on rank 0; NULL if world_size==1 */
    /* DREAM kwargs (dream.py:20-27) */
    double gamma_scale; /* 1.0 */
    int32_t del_pairs;  /* 3; 1 ... 10 */
    int32_t burnin_gen; /* 300 */
    int32_t n_cr_gen;   /* 50 */
    int32_t n_cr;       /* 3, <= BPM_MAX_CR */
    /* build-defined extensions (absent from the reference) */
    double p_snooker;      /* DE-MC only: probability of a snooker update (0 = off) */
    int32_t outlier_every; /* DREAM burn-in: IQR outlier-chain reset every this many generations (0 = off) */
    int32_t keep_history;  /* 1: append every generation (chain.py:51-54); 0: keep current state only */
    int32_t running_moments; /* 1: keep, per generation, the population sums sum_i x_ij and sum_i x_ij^2 (2 dim doubles): bpm_reduce_moments
                              * then answers for any burn-in of WHOLE generations without a resident history -- param_est (demc.py:235-248)
                              * of 10^5 generations of config 2 would otherwise need 660 GB.  Two small dispatches per generation. */
    int32_t _pad2;
} bpm_config_t;

/* run_mcmc(**kwargs) (demc.py:73-75,161-162; dream.py:40-41). */
typedef struct bpm_run_opts {
    double flip;      /* 0.5; clipped to [0,1] */
    int32_t shuffle;  /* 1 */
    int32_t _pad;
    double epsilon;   /* < 0: default (DE-MC 1e-15, DREAM 1e-12); std of the normal jitter */
    double u_epsilon; /* < 0: default 1e-2 (DREAM uniform jitter half-width) */
    double gamma;     /* <= 0: default 2.38/sqrt(2 dim) (DE-MC only) */
} bpm_run_opts_t;

typedef struct bpm_stats {
    int64_t local_n_accepted; /* demc.py:67,190 (this run, this rank) */
    int64_t local_n_rejected; /* demc.py:68,193: starts at 1 */
    int64_t n_nan_alpha;      /* updates whose Metropolis ratio was NaN (reference raises ValueError) */
    int64_t k_gen;            /* generations done in the current run (demc.py:78,134) */
    int64_t t_abs;            /* generations done since creation */
    int64_t history_rows;     /* generations stored + 1 (row 0 = initial state) */
    int64_t n_outlier_resets;
    int32_t n_cr;
    int32_t _pad;
    double p_cr[BPM_MAX_CR];         /* dream.py:114 */
    double delta_m[BPM_MAX_CR];      /* dream.py:117 */
    double n_cr_updates[BPM_MAX_CR]; /* dream.py:115 */
} bpm_stats_t;

const char* bpm_last_error(void);
int bpm_abi_version(void);
/* Provenance: the first 16 hex digits of the SHA-256 over the sources this binary was built from (bipymc_amd/csrc/Makefile: ID_SRCS), baked in at
 * compile time.  The binding recomputes it from the tree and refuses a stale library; profiles/traffic_*.json carry the id the counters were taken
 * on.  (No counterpart in the reference: pure Python has no build.) */
const char* bpm_build_id(void);
/* GPUs visible to this process (hipGetDeviceCount): what one rank per GPU needs to pick its device where the reference
 * picks nothing (mpi4py ranks share the host's cores, demc.py:15). */
int bpm_device_count(int32_t* out);

/* rank 0 calls this and ships the bytes to the other ranks (mpi4py bcast / torch.distributed). */
int bpm_get_unique_id(char out[BPM_UID_BYTES]);

int bpm_create(const bpm_config_t* cfg, bpm_handle_t* out);
/* Non-zero when the library's own AQL queue had failed (a wait ran into its limit) and could not be quiesced: the handle is gone, but
 * its device buffers were deliberately leaked instead of freed under kernels that may still run (bpm_last_error says so). */
int bpm_destroy(bpm_handle_t h);

/* McmcChain.__init__ for every chain (chain.py:25-27): state0 = theta_0 + N(0, diag(varepsilon)),
 * varepsilon = VARIANCES, length dim (all > 0, else no jitter: util.py:12).  History := [state0]. */
int bpm_init_chains(bpm_handle_t h, const double* theta_0, const double* varepsilon);
/* Set the (N, dim) state matrix in global-id order (warm start, demc.py:46-51).  History := [X]. */
int bpm_set_state(bpm_handle_t h, const double* X);
int bpm_get_state(bpm_handle_t h, double* X);
/* Warm start with full histories (demc.py:46-51,217-233; chain.py:82-93): hist_local is
 * (rows, n_local, dim) for this rank's chains, X the (N, dim) current state of all chains. */
int bpm_set_history(bpm_handle_t h, int64_t rows, const double* hist_local, const double* X);
/* cached ln_like of the current state.  bpm_set_loglike: HOST-CALLBACK targets only (they must set the n_local local values after every
 * (re)initialisation; a sampler with a device target evaluates them itself and refuses the call). */
int bpm_set_loglike(bpm_handle_t h, const double* ll_local); /* n_local values */
int bpm_get_loglike(bpm_handle_t h, double* ll_local);

/* _mcmc_run prologue (demc.py:67-78): counters reset, k_gen = 0, kwargs latched. */
int bpm_begin_run(bpm_handle_t h, const bpm_run_opts_t* opts);
/* n_gens iterations of the while loop of demc.py:79-140, entirely on the device. Asynchronous. */
int bpm_step(bpm_handle_t h, int64_t n_gens);
/* same, synchronous, timed on the device with two HIP events BOUND TO UPDATE-KERNEL DISPATCHES of the sampler's stream (no
 * marker packets: an event-record pair alone costs ~17 us here, 7 % of a 20-generation window): elapsed_ms = end of update
 * launch number n/4 (the first one when n_gens < 8: binding an event costs the host 10-30 us, which a call starting from an
 * idle GPU can only absorb once the host runs ahead) -> end of the last one, n_launches = the launches that interval covers.
 * Average launch period = elapsed_ms / n_launches. */
int bpm_step_timed(bpm_handle_t h, int64_t n_gens, float* elapsed_ms, int64_t* n_launches);
/* the figures of the last bpm_step_timed call (which may be given NULL, NULL: reading the events costs tens of microseconds of
 * host time that a caller timing the call with its own clock does not want inside) */
int bpm_get_step_time(bpm_handle_t h, float* elapsed_ms, int64_t* n_launches);
int bpm_synchronize(bpm_handle_t h);
/* Exchange policy for world_size > 1: what the Allgather of demc.py:93-94,116-117 moves.  Outside DREAM's CR
 * adaptation (where delta / cr_idx of every chain travel with the dense block) a half generation only changes the rows
 * that were ACCEPTED, and everything a proposal is made of -- the replicated state matrix, counter-addressed draws,
 * update records -- is on every rank already.  mode 2 (default), "replay": owners all-gather ONE BYTE per local chain
 * (accepted or not) and every rank recomputes the other ranks' accepted proposals into its replica with the update
 * kernel's own proposal code (bit-identical by construction).  mode 1, "rows": ranks all-gather fixed-capacity packed
 * blocks (up to 4 sub-blocks [count | ids | rows] per rank) and scatter them; generations run in chunks of 64 under a
 * device-side checkpoint, a chunk in which a sub-block overflowed is rolled back and repeated with mode 0; cap > 0
 * sets the capacity (rows per sub-block per half generation) of the next chunk, afterwards it follows the largest
 * count seen.  mode 0: the dense all-gather of whole blocks.  The same values on every rank. */
int bpm_set_exchange(bpm_handle_t h, int32_t mode, int32_t cap);
/* out[8] = {mode, current capacity of mode 1, chunks run with mode 1, chunks of mode 1 repeated dense,
 *           generations exchanged by replay, generations exchanged by push, bits 0-1: 1 if the push exchange is connected (2: with the
 *           control block in fine-grained memory of its own) | bit 2 / bit 3: the arena probe of bpm_push_selftest passed with system- /
 *           agent-scope packet fences | bit 4: it ran on the library's own queue,
 *           barriers so far | bit 62 when the push exchange fences at agent scope} */
int bpm_get_exchange_stats(bpm_handle_t h, int64_t* out);
/* mode 3, "push" (the default once connected): where the reference's ranks meet in MPI_Allgather twice per generation
 * (demc.py:93-94,116-117), the OWNER of a chain stores an accepted row -- during CR adaptation also every update's (delta, cr)
 * statistic, dream.py:92 -- straight into every other rank's replica of the state matrix from inside the update kernel: the ranks'
 * exchange buffers are mapped into each other's address space (hipIpcOpenMemHandle; peer memory over xGMI on a multi-GPU node).  A
 * one-wavefront kernel per half generation announces "done" in every peer's control block and waits for the peers' announcements; no
 * collective, no recomputation, and the rank's kernels run on the library's own queue like a single-GPU sampler's.
 * cap (mode 3): 0 = the update kernels' packets acquire and release at SYSTEM scope, what the HSA memory model asks for between agents
 * (default); 1 = at AGENT scope, 6 us less per half generation on MI355X -- the pushed rows themselves are system-scope write-through
 * stores either way; whether the cheaper fences suffice between the GPUs of a node is a property of the platform that a caller
 * verifies by comparing the ranks' replicas (bench.py does, before it times anything).
 *   bpm_push_export   blob[BPM_PUSH_BLOB_BYTES]: what the other ranks need to map this rank's buffer
 *   bpm_push_connect  blobs = the exports of ALL ranks in rank order (world_size x BPM_PUSH_BLOB_BYTES), moved by the caller's own
 *                     communicator (the reference's counterpart is mpi_comm itself, demc.py:15)
 *   bpm_push_selftest collective; handles = this process's ranks (one, or the R ranks of a local test group).  (1) every rank writes a pattern
 *                     into every peer's control block, one barrier, every rank checks; (2) every rank stores probe rows into ITS block of
 *                     every peer's arena (first and last row, the block's last slots, both ends of its outlier block: where its update
 *                     kernels will push) from the queue and under the packet fences the update kernels use, a barrier, every rank verifies
 *                     what arrived and restores what was there -- with system-scope fences (*ok = (1) and this), then with the agent-scope
 *                     form (bpm_get_exchange_stats out[6] bit 3).  A mapping that points elsewhere, or stores that are not visible behind
 *                     the hand-over, end as *ok = 0 (-> an RCCL exchange), not as a fault or a divergence in the first generation.
 *   bpm_destroy       of a connected rank of a world of processes announces "closing" to its peers and waits, bounded
 *                     (BPM_PUSH_CLOSE_TIMEOUT_S, default 3 s), for theirs before it unmaps and frees: the library orders the teardown, the
 *                     caller needs no barrier of its own.  A rank that still exchanges with a closed rank gets an error at its next
 *                     bpm_synchronize ("closed its sampler") instead of waiting for its time limit.
 * A sampler created with a nccl_uid that starts with "BPMPUSH" has no RCCL communicator at all (ranks sharing one GPU, which RCCL
 * refuses; nodes without RCCL): the push exchange is then its only one.  Every rank must enter bpm_step within BPM_PUSH_TIMEOUT_S
 * (default 30) seconds of the others; a rank that waited longer reports it at the next bpm_synchronize. */
int bpm_push_export(bpm_handle_t h, void* blob);
int bpm_push_connect(bpm_handle_t h, const void* blobs);
int bpm_push_selftest(bpm_handle_t* handles, int32_t R, int32_t* ok);
/* How the generation loop's kernels reach the GPU (no counterpart in the reference: its loop is the Python interpreter,
 * demc.py:79-140).  A sampler with a device target dispatches its generation loop through the library's own user-mode AQL queue
 * (packets written by the library, bipymc_amd/csrc/aql_queue.h) -- update kernels, table builds, the CR reduction kernels of burn-in,
 * with the push exchange also the cross-rank barrier kernels of a rank of a world; RCCL exchanges and every other entry point use the
 * HIP stream.  out[6] = {1 if the sampler has such a queue, update-kernel dispatches of the calling thread through it, update-kernel
 * launches of the calling thread through the HIP stream, 1 if work may be in flight on the queue, 0 (was: experimental memory type),
 * packet fences of the update kernels on the queue: 3 acquire + release, 1 acquire only (the default: what later kernels read leaves
 * through write-through stores)}.
 * BPM_DIRECT_QUEUE=0 in the environment disables the queue. */
int bpm_get_launch_stats(bpm_handle_t h, int64_t* out);
/* direct != 0: use the library's own queue where the sampler has one (the default); 0: HIP stream launches only.
 * fence: packet fences of the update kernels on that queue: -1 keep, 3 agent-scope acquire + release on every packet with plain
 * stores (what a HIP stream does), 1 acquire only with write-through stores of what later kernels read (the default where the queue
 * exists); 0 is refused (fence-less packets belong to an experiment build only).  Results do not depend on the
 * launch path (tested). */
int bpm_set_launch_path(bpm_handle_t h, int32_t direct, int32_t fence);
/* Host-callback ln_like_fn (samplers.py:36-43): one half generation = propose + commit.
 * bpm_propose writes the proposals of this rank's chains of the current phase into out_prop
 * (n_out rows of dim) and their global ids into out_ids (capacity n_local each); the caller evaluates
 * ln_like_fn row by row and hands the values to bpm_commit, which does the Metropolis test
 * (samplers.py:328-336), the append (chain.py:51-54) and, after the second phase, k_gen += 1. */
int bpm_propose(bpm_handle_t h, double* out_prop, int32_t* out_ids, int32_t* n_out);
int bpm_commit(bpm_handle_t h, const double* ll_prop);
/* The same half generation with the read-back OVERLAPPED with the caller's evaluation (round 5).  bpm_propose_begin launches the proposal kernel and
 * queues the device-to-host copies of the proposals in n_chunks pieces (1 ... 256) into pinned staging OF THE LIBRARY, then returns at once;
 * bpm_propose_chunk(k) waits for piece k only and returns pointers INTO that staging -- *n_rows rows of *ld doubles (the first dim are the proposal;
 * ld = dim rounded up to even) in work-item order and their global chain ids (-1: an idle work item of a rank of a world; its value is ignored) --
 * valid until bpm_commit_end: while the caller evaluates ln_like_fn on piece k (samplers.py:36-43) the DMA of the following pieces proceeds.
 * bpm_commit_chunk(k, ll) hands in the *n_rows values of piece k (any order of k; the library copies), bpm_commit_end does what bpm_commit does.
 * bpm_propose_chunk -- and only it -- may be called from several host threads at once (a pool evaluating the pieces in parallel). */
int bpm_propose_begin(bpm_handle_t h, int32_t n_chunks);
int bpm_propose_chunk(bpm_handle_t h, int32_t k, const double** rows, const int32_t** ids, int32_t* n_rows, int32_t* ld);
int bpm_commit_chunk(bpm_handle_t h, int32_t k, const double* ll);
int bpm_commit_end(bpm_handle_t h);
/* ... and with the likelihood evaluated ON THE DEVICE by the caller's own framework (a vectorised torch / cupy likelihood): nothing crosses PCIe.
 * bpm_propose_device returns, complete, *rows_dev = DEVICE pointer to the half generation's *n_rows proposal rows of *ld doubles (work-item order)
 * and *ids_dev = device pointer to their global chain ids (-1: idle work item); bpm_commit_device takes a DEVICE pointer to *n_rows float64 values
 * in the same order (memory of this sampler's GPU; the library waits for the whole device first -- the values may come from any stream -- and
 * copies them).  bpm_state_device / bpm_set_loglike_device are the device-resident forms of bpm_get_state (local chains only: n_local rows where
 * they lie, read-only) + bpm_set_loglike, needed once per (re)initialisation. */
int bpm_propose_device(bpm_handle_t h, const double** rows_dev, const int32_t** ids_dev, int32_t* n_rows, int32_t* ld);
int bpm_commit_device(bpm_handle_t h, const double* ll_dev);
int bpm_state_device(bpm_handle_t h, const double** rows_dev, int32_t* n_rows, int32_t* ld);
int bpm_set_loglike_device(bpm_handle_t h, const double* ll_dev);
/* ... and with the likelihood given as HIP SOURCE (round 5; samplers.py:36-43 takes any Python callable -- this is the form of it that runs at device
 * speed with no framework in the process): `hip_source` defines
 *     __device__ double ln_like(const double* x, int d, const double* p)       (x: one parameter vector; p: the caller's parameter block = ln_kwargs)
 * (or, per coordinate: `#define BPM_LN_LIKE_TERMS K` + ln_like_terms(xj, j, d, p, acc) adding coordinate j's contribution to K <= 8 sums +
 * ln_like_finish(acc, d, p): inside the update kernel every lane of a chain then adds its own coordinates' terms; bipymc_amd/csrc/user_likelihood.h)
 * bpm_set_device_likelihood compiles it with hiprtc (loaded on demand) into one kernel -- a thread per proposal row -- that runs between the library's
 * proposal and commit kernels, copies the n_params doubles of `params` to the device and evaluates the current states (what bpm_set_loglike takes from
 * the host).  From then on bpm_step drives this host-callback sampler like one with a shipped target: no host code inside a generation.  f64 arithmetic
 * is compiled unfused (-ffp-contract=off) like the library's own.  A source that does not compile: error, the compiler's log in bpm_last_error.
 * bpm_refresh_device_loglike re-evaluates the current states (after bpm_set_state / bpm_init_chains / a warm start).
 * bpm_check_device_likelihood compiles only (no sampler, no GPU needed; arch NULL = "gfx950"): 0 or -1 with the reason in `log` (and bpm_last_error). */
int bpm_set_device_likelihood(bpm_handle_t h, const char* hip_source, const double* params, int32_t n_params);
int bpm_refresh_device_loglike(bpm_handle_t h);
int bpm_check_device_likelihood(const char* hip_source, const char* arch, char* log, int64_t log_cap);
/* bpm_set_device_likelihood also compiles the UPDATE KERNEL ITSELF around the caller's function (the library carries its kernel source; rows of up to
 * 512 coordinates): bpm_step then needs one launch per half generation instead of three (proposal / likelihood / commit).  Whatever fails on that way
 * leaves the three-kernel form in use: *fused says which runs, `why` (up to why_cap - 1 characters, may be NULL) why not the fused one.
 * The module's kernels are dispatched like the library's own (its AQL queue finds them by name).  Environment: BPM_USER_FUSED=0 does not attempt the
 * fused form, =2 launches it on the HIP stream (A/B). */
int bpm_get_device_likelihood_info(bpm_handle_t h, int32_t* fused, char* why, int64_t why_cap);
/* The PER-DATUM form (samplers.py:36-43 takes any callable; the reference's fitting scripts sum over their data points inside it): `hip_source` says
 * `#define BPM_LN_LIKE_DATA K` (1 ... 8 sums) and `#define BPM_LN_LIKE_DATA_W w`, and defines
 *     __device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc)      (y: the w values of datum i)
 *     __device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p)          (x: for a prior)
 * (the form is recognised by the source's own directive line `#define BPM_LN_LIKE_DATA K`, blanks as the preprocessor allows them; the name in a comment
 * does not count; bpm_set_device_likelihood refuses such a source, this entry refuses one without it)
 * `data`: (n_data, w) row-major, 1 <= n_data < 2^31, 1 <= w <= 64, copied to the device here and kept until the likelihood is replaced or the handle
 * destroyed.  A wavefront per (row, chunk of the data) adds the terms, in an order that depends on n_data alone: a row's value is a function of
 * (x, data, params), bit for bit (bipymc_amd/csrc/user_eval_data.h).  Never fused (bpm_get_device_likelihood_info says so); a single rank only. */
int bpm_set_device_likelihood_data(bpm_handle_t h, const char* hip_source, const double* params, int32_t n_params, const double* data, int64_t n_data,
                                   int32_t w);
/* samplers.py:36-43: ln_like_fn(theta) at n given points X (n, dim) -- the installed device likelihood of any form, by its kernel of its own
 * (bpm_eval_loglike is the same for the shipped targets).  Error when none is installed. */
int bpm_eval_device_likelihood(bpm_handle_t h, const double* X, int32_t n, double* out);
/* samplers.py:36-43 (the per-datum form of ln_like_fn): the number of consecutive data points one wavefront sums; with n_data it fixes the order of the additions */
int bpm_data_likelihood_chunk(void);

/* history of this rank's chains: out[(g - g_lo) * n_local * dim + i * dim + j], g in [g_lo, g_hi) */
int bpm_get_history(bpm_handle_t h, int64_t g_lo, int64_t g_hi, double* out);
int bpm_get_loglike_history(bpm_handle_t h, int64_t g_lo, int64_t g_hi, double* out);
/* Room for total_rows STORED rows.  The growth is checked against the free device memory before anything is allocated (while the old rows are
 * copied the old and the new buffer exist at once); the refusal states the size needed and names the ways out -- a thinned history (below), or
 * keep_history = 0 with running_moments -- and leaves the handle usable.  Every step call reserves the rows it will store the same way. */
int bpm_reserve_history(bpm_handle_t h, int64_t total_rows);
/* THINNED HISTORIES (build-defined; the reference's McmcChain appends every generation, chain.py:51-54, and has no thinning).  A history has
 * a stride k >= 1: stored row r is logical row r k, where logical row t is the state after generation t since the last (re)initialisation
 * (row 0 = the initial state), and a generation is appended iff the logical row it produces is a multiple of k.  A thinned run's history is
 * exactly [::k] of the dense run's from the same seed; state, ln-likes, accept counters, p_cr, delta_m and the CR adaptation of burn-in are
 * bit-identical to the dense run's, and with stride 1 nothing changes at all.  Every statistic of the history (bpm_reduce_moments,
 * bpm_diag_*, bpm_quantile_*, bpm_reduce_cov, bpm_hist_*, bpm_trace_*, bpm_derive) counts STORED rows: n_burn, g_lo / g_hi, every and lags.
 * bpm_set_history_thin: what chain.py:51-54 appends, thinned to every k-th generation from now on.  Allowed while the history holds only its
 *   initial row (after bpm_create / bpm_init_chains / bpm_set_state), or when k is the current stride; otherwise an error that points to
 *   bpm_thin_history.  The stride belongs to the handle and survives bpm_init_chains / bpm_set_state (bpm_set_history installs a row per
 *   generation: stride 1).  Refused, each with its reason: k < 1; keep_history = 0 with k > 1; running_moments = 1 with k > 1 (those sums count every
 *   generation: the two n_burn units would disagree); outlier_every > 0 with k > 1 (the outlier check reads a row per generation).
 * bpm_thin_history: thins what chain.py:51-54 has appended so far: keeps stored rows 0, m, 2m, ... and their ln-like rows; the new stride is
 *   the old one times m, the new row count (rows - 1) / m + 1; m = 1 is a no-op.  Recording stays aligned by the append rule.  The kept rows
 *   are gathered into new buffers of exactly that size, which replace the old ones; the old memory is returned, and an error on the way
 *   leaves the sampler as it was.  Rows kept in position order stay so.  Open bpm_quantile_* / bpm_hist_* / bpm_trace_* / bpm_diag_* windows
 *   answer "the history changed" afterwards.  The same refusals, and: a stride beyond 2^31 - 1, a half generation open (bpm_propose).
 * bpm_set_history_thinned: warm start from a thinned checkpoint (chain.py:51-54's rows, every k-th): bpm_set_history, then stride k and the
 *   logical length rows_logical; rows must be (rows_logical - 1) / k + 1.  X is the CURRENT state, which is the last row only when
 *   (rows_logical - 1) % k == 0; otherwise every stored row, a single one included, is hist_local's.  An error behind the checks of the
 *   arguments leaves the handle as a failed bpm_set_history does: re-initialised at X with one row, its stride kept.
 * bpm_get_history_thin: out = {stride, logical rows, stored rows, logical index of the last stored row}. */
int bpm_set_history_thin(bpm_handle_t h, int32_t k);
int bpm_thin_history(bpm_handle_t h, int32_t m);
int bpm_set_history_thinned(bpm_handle_t h, int64_t rows, const double* hist_local, const double* X, int32_t k, int64_t rows_logical);
int bpm_get_history_thin(bpm_handle_t h, int64_t out[4]);
/* param_est (demc.py:235-248) without moving the history: for this rank's rows of the interleaved
 * super chain (row g*N + i = chain i at generation g) with row index >= n_burn, returns count,
 * sum_j (x - shift_j), sum_j (x - shift_j)^2 and shift_j (length dim each; shift is identical on every
 * rank).  mean_j = shift_j + S1/n, var_j = S2/n - (S1/n)^2 after summing S1, S2, n over ranks.  A sampler created with
 * running_moments and without a resident history answers from its per-generation sums: n_burn must then be a multiple of n_chains. */
int bpm_reduce_moments(bpm_handle_t h, int64_t n_burn, double* sum, double* sumsq, double* shift, int64_t* count);
int bpm_get_stats(bpm_handle_t h, bpm_stats_t* out);
/* checkpoint what the reference forgets: p_cr, delta_m, n_cr_updates, t_abs */
int bpm_set_adapt_state(bpm_handle_t h, const double* p_cr, const double* delta_m, const double* n_cr_updates,
                        int64_t t_abs);

/* ln_like of n points (row-major (n, dim)) with the sampler's device target: what `ln_like_fn(theta)` returns for the shipped analytic
 * targets (utils/d100_gauss.py:14-35, dblgauss_rv.py:11-32, banana_rv.py:11-40) */
int bpm_eval_loglike(bpm_handle_t h, const double* X, int32_t n, double* out);

/* Split-chain moments of this rank's chains over history rows [g_lo, g_hi) (convergence diagnostics; absent from the reference).
 * n = (g_hi - g_lo) / 2 draws per half-chain: rows [g_lo, g_lo + n) and [g_hi - n, g_hi) of every chain (the middle row of an odd window is
 * dropped), 2 n_local half-chains.  Per coordinate (dim values each): mean of the half-chain means, sum of squared deviations of the
 * half-chain means from it, sum of the half-chain variances (ddof 1).  Keeps the half-chain means on the device for bpm_diag_autocov.
 * Errors: no resident history (keep_history = 0), n < 4.  bipymc_amd/diagnostics.py combines ranks and finishes R-hat and ESS. */
int bpm_diag_split_moments(bpm_handle_t h, int64_t g_lo, int64_t g_hi, double* mean_of_means, double* m2_of_means,
                           double* sum_of_vars, int64_t* n_half_chains, int64_t* n_draws);
/* sum over this rank's half-chains of c_{j,t} = (1/n) sum_{i < n - t} (x_{j,i} - xbar_j)(x_{j,i+t} - xbar_j), t in [t0, t0 + n_lags),
 * out[(t - t0) * dim + k]; window of the last bpm_diag_split_moments call, which must still describe the resident history (an error after
 * a step, bpm_set_history or bpm_set_state); t0 + n_lags <= n. */
int bpm_diag_autocov(bpm_handle_t h, int64_t t0, int32_t n_lags, double* out);

/* Exact quantiles of the super chain on the device (what `np.quantile(param_est(n_burn)[2], q, axis=0)` computes on the host after
 * gathering the history, and the 5/50/95 percentiles the reference prints, mc_plot/vis_mcmc_chains.py:76): the histograms of an MSD radix
 * select over order-preserving 64-bit keys (negative -> all bits flipped, else sign bit set, every NaN -> ~0); bipymc_amd/quantiles.py
 * runs the select across ranks and NumPy's linear interpolation.
 * bpm_quantile_begin fixes the window -- super-chain rows >= n_burn, a partial first generation by chain index, as bpm_reduce_moments --
 * and returns this rank's number of rows in it.  Errors: no resident history (keep_history = 0). */
int bpm_quantile_begin(bpm_handle_t h, int64_t n_burn, int64_t* count);
/* n_prefix slots (prefix_dim[j], prefixes[j]), sorted by coordinate, prefixes of a coordinate strictly increasing, each of prefix_bits bits
 * (0, 8, ..., 56).  hist[j * 256 + b] = keys of coordinate prefix_dim[j] in the window whose top prefix_bits bits are prefixes[j] and whose
 * next 8 bits are b; n_nan[j] (may be NULL) = how many of them are NaN.  An error once the history changed since bpm_quantile_begin (a
 * step, bpm_set_history or bpm_set_state). */
int bpm_quantile_histogram(bpm_handle_t h, int64_t n_prefix, const int32_t* prefix_dim, const uint64_t* prefixes, int32_t prefix_bits,
                           uint64_t* hist, int64_t* n_nan);
/* Centred sums of the super chain on the device (posterior covariance; the reference looks at it through corner.corner over the gathered
 * samples, mc_plot/mc_plot.py:16-29): over this rank's rows of the window of bpm_reduce_moments (super-chain rows >= n_burn, a partial first
 * generation by chain index), sum[k] = sum (x_k - center_k) (dim values) and cross[i * dim + j] = sum (x_i - center_i)(x_j - center_j)
 * (dim x dim, row-major, full and exactly symmetric), count = the rows.  FP64 matrix-core SYRK over the resident history; per-workgroup
 * partial sums are added in a fixed order, so the same history gives the same bits.  Keeps no state between calls and writes nothing the
 * samplers read.  bipymc_amd/covariance.py centres on the global mean, merges the ranks and finishes cov = (S2 - S1 S1^T / n) / (n - 1).
 * Errors: no resident history (keep_history = 0); dim beyond 16384, or a dim x dim result and partial sums larger than the free device
 * memory (the message names the limit). */
int bpm_reduce_cov(bpm_handle_t h, int64_t n_burn, const double* center, double* sum, double* cross, int64_t* count);
/* Marginal and pairwise histograms of the super chain on the device: the counts of the reference's corner plot (corner.corner(samples),
 * mc_plot/mc_plot.py:16-29: a 1-D histogram per parameter, a 2-D histogram per pair), taken over the resident history.
 * bpm_hist_range fixes the window of bpm_reduce_moments (super-chain rows >= n_burn, a partial first generation by chain index) and returns,
 * per coordinate over this rank's rows of it, lo / hi = the smallest / largest value that is not NaN (+inf / -inf where there is none), n_nan
 * and n_inf = how many values are NaN / infinite (dim values each), count = the rows.  The caller (bipymc_amd/histograms.py) merges the
 * ranks, applies NumPy's range rules and builds the edges with np.linspace; the device receives edges only.
 * bpm_hist_marginals: counts[j * bins + i] = rows of that window whose coordinate dims[j] lies in bin i of the bins + 1 non-decreasing edges
 * edges[j * (bins + 1) ...]: e[i] <= x < e[i + 1], the last bin also x == e[bins]; NaN and values outside are counted nowhere -- exactly
 * np.histogram's counts for these edges (a guessed bin is corrected against the edges).  1 <= bins <= 1024; dims: n_dims coordinates.
 * bpm_hist_pairs: counts2d[(p * bins2d + i) * bins2d + j] = rows whose coordinate dims[pair_a[p]] lies in bin i of edges2d[pair_a[p]] and
 * whose coordinate dims[pair_b[p]] lies in bin j of edges2d[pair_b[p]] (pair_a, pair_b index dims; edges2d: n_dims x (bins2d + 1)) -- exactly
 * np.histogram2d's counts.  1 <= bins2d <= 64, 1 <= n_pairs <= 2^24.
 * Counts are integers added by integer atomics: the same history gives the same bits, ranks merge by addition.  The two counting calls
 * return an error once the history changed since bpm_hist_range (a step, bpm_set_history or bpm_set_state).  Every device buffer is
 * temporary; nothing the samplers read is written.  Errors: no resident history (keep_history = 0); bins / bins2d / n_pairs beyond the
 * limits, or counts and temporaries larger than the free device memory (the message names the limit). */
int bpm_hist_range(bpm_handle_t h, int64_t n_burn, double* lo, double* hi, int64_t* n_nan, int64_t* n_inf, int64_t* count);
int bpm_hist_marginals(bpm_handle_t h, int32_t n_dims, const int32_t* dims, int32_t bins, const double* edges, int64_t* counts);
int bpm_hist_pairs(bpm_handle_t h, int32_t n_dims, const int32_t* dims, int32_t bins2d, const double* edges2d, int64_t n_pairs,
                   const int32_t* pair_a, const int32_t* pair_b, int64_t* counts2d);
/* Per-generation trace summaries of the resident history on the device: what the reference's trace plots draw from the gathered chains
 * (plot_mcmc_indep_chains / plot_mcmc_chain, mc_plot/mc_plot.py:52-102: one line per chain, np.mean and np.std per generation; the reason
 * its examples call param_est(n_burn=0) a second time), without moving the history.
 * bpm_trace_bins: bins t = 0 .. T - 1, T = ceil((g_hi - g_lo) / every), of the history rows [g_lo + t every, min(g_lo + (t + 1) every, g_hi))
 * pooled over this rank's chains (every larger than the range: one bin).  Per bin and coordinate, bin_counts = [2][T][dim]: how many values
 * are finite | NaN; bin_sums = [5][T][dim]: a shift c (a finite value of the bin: the rank's first row of it where that is finite) | sum (x - c)
 * | sum (x - c)^2 over the finite values | min | max over the values that are not NaN (+inf / -inf where there is none; infinite values show
 * here only).  The same over the ln-like history, ll_counts = [4][T]: finite | NaN | +inf | -inf, ll_sums = [5][T].  best_ll / best_row /
 * best_x (dim values): the largest ln-like of the range that is not NaN, the smallest local row g * n_local + i that carries it, and that
 * row's state (NaN, -1, NaN where every ln-like is NaN).  One pass over the range; every partial result is merged in a fixed order and
 * there is no floating-point atomic, so the same history gives the same bits.  bipymc_amd/traces.py merges the ranks (mean = c + S1 / n,
 * M2 = S2 - S1^2 / n, Chan's formula) and finishes mean and sd.
 * bpm_trace_chains: the local chains local_ids[0 .. n) at the first history row of every bin of the last bpm_trace_bins:
 * out_x[(t * n + j) * dim + k], out_ll[t * n + j].  An error once the history changed since bpm_trace_bins (a step, bpm_set_history or
 * bpm_set_state).  Every device buffer is temporary; nothing the samplers read is written (a history kept in position order is put into
 * chain order first, as bpm_get_history does).  Errors: no resident history (keep_history = 0), a range outside the history, every < 1,
 * a chain outside [0, n_local), records larger than the free device memory (the message names the requirement). */
int bpm_trace_bins(bpm_handle_t h, int64_t g_lo, int64_t g_hi, int64_t every, int64_t* bin_counts, double* bin_sums, int64_t* ll_counts,
                   double* ll_sums, double* best_ll, int64_t* best_row, double* best_x);
int bpm_trace_chains(bpm_handle_t h, int32_t n, const int32_t* local_ids, double* out_x, double* out_ll);
/* Posterior summaries of a caller's DERIVED QUANTITIES on the device: what the reference's fitting scripts do on the host with
 * param_est(n_burn)[2] (examples/ex_exp_fit.py:197-202: c_0 / c_inf per sample, its mean and standard deviation; :176-192: the fitted model
 * at every sample for the trajectory picture; ex_line_fit.py and ex_para_fit.py likewise), without moving the history.  `hip_source` defines
 *     __device__ void derive(const double* x, int d, double ll, const double* p, double* out)
 * (x: one super-chain row of d coordinates; ll: its stored ln-like; p: the caller's parameter block; out[0 .. n_out), 1 <= n_out <= 256: zero
 * on entry, so an output the function does not write is 0.0; device math functions, INFINITY, NAN and M_PI as for ln_like; compiled -O3
 * -ffp-contract=off).  The library compiles one window-reduction kernel around it with hiprtc (bipymc_amd/csrc/derived.h).
 * bpm_check_device_function compiles only (no sampler, no GPU needed; arch NULL = "gfx950"): 0 or -1 with the reason in `log` (and
 * bpm_last_error).  bpm_set_device_function compiles for the handle's device, loads the module and copies the n_params doubles of `params`;
 * the handle keeps the module until another function replaces it or bpm_destroy.  The same source bytes and n_out again reuse the loaded
 * module and only copy `params`.  Any sampler may carry one, whatever its target.
 * bpm_derive: over this rank's super-chain rows >= n_burn (bpm_reduce_moments' selection: a partial first generation by chain index), per
 * output m: counts = [2][n_out]: how many values are finite | NaN; sums = [5][n_out]: a shift c (a finite value of the output) | sum (v - c) |
 * sum (v - c)^2 over the finite values | min | max over the values that are not NaN (+inf / -inf where there is none) -- bpm_trace_bins'
 * records; *n_rows: the window's local rows, *n_first: how many of them belong to a partial first generation (0: whole generations only).
 * values (may be NULL): values[r * n_out + m] = output m of the window's r-th local row, n_rows * n_out doubles, values_cap: what the buffer
 * holds.  Every partial result is merged in a fixed order and there is no atomic: the same history gives the same bits.
 * bipymc_amd/derived.py merges the ranks (traces.py: merge_moments / finish) and puts the values into super-chain order.
 * Every device buffer is temporary; nothing the samplers read is written (a history kept in position order is put into chain order first,
 * as bpm_get_history does).  Errors: n_out out of range, a source that does not compile (the compiler's log in bpm_last_error), no function
 * installed, n_burn < 0, no resident history (keep_history = 0), values beyond values_cap or of 2^31 elements or more, records or values
 * larger than the free device memory (the message names the requirement). */
int bpm_check_device_function(const char* hip_source, int32_t n_out, const char* arch, char* log, int64_t log_cap);
int bpm_set_device_function(bpm_handle_t h, const char* hip_source, int32_t n_out, const double* params, int32_t n_params);
int bpm_derive(bpm_handle_t h, int64_t n_burn, int64_t* counts, double* sums, int64_t* n_rows, int64_t* n_first, double* values,
               int64_t values_cap);
/* WAIC AND THE POINTWISE LOG PREDICTIVE DENSITY on the device: which of two models predicts the data better.  The reference has no such
 * statistic; its fitting scripts sum a log density over their data points inside ln_like_fn (examples/ex_line_fit.py:63-67).  Here ONE term of
 * that sum is the caller's, `hip_source` defines
 *     __device__ double ln_like_point(const double* x, int d, const double* y, int i, const double* p)
 * (x: one super-chain row of d coordinates; y: the w values of datum i, 1 <= w <= 64; p: the caller's parameter block; device math functions,
 * INFINITY, NAN and M_PI as for ln_like; compiled -O3 -ffp-contract=off), and the library compiles a streaming reduction around it with hiprtc
 * whose parallel axis is the data (bipymc_amd/csrc/pointwise.h, pointwise_rows.h): a thread per datum meets the window's rows in ascending order
 * and keeps, in registers, an online log-sum-exp and the shifted moments of its values l.
 * bpm_check_pointwise compiles only (no sampler, no GPU needed; arch NULL = "gfx950"): 0 or -1 with the reason in `log` (and bpm_last_error).
 * bpm_set_pointwise compiles for the handle's device, loads the module, copies `data` ((n_data, w) float64 row-major, 1 <= n_data < 2^31) to
 * the device once and the n_params doubles of `params`; the handle owns all three until another function replaces them or bpm_destroy.  The
 * same source bytes, w and data contents again keep module and data and only copy `params` (*reused, may be NULL: 1 then, else 0).  Any
 * sampler may carry one, whatever its target or likelihood.
 * bpm_pointwise: over this rank's super-chain rows >= n_burn (bpm_reduce_moments' selection), per datum i: records = [9][n_data], field f of
 * datum i at records[f * n_data + i]: 0 the count n of finite l (64-bit word) | 1 a shift c (the first finite l) | 2 sum (l - c) | 3 sum
 * (l - c)^2 over the finite l | 4, 5, 6 how many l are NaN, +inf, -inf (64-bit words) | 7 m, the largest finite l | 8 s = sum exp(l - m) over
 * the finite l (their log-sum-exp is m + log s; m = -inf, s = 0 where n = 0).  *n_rows, *n_first, values (values[r * n_data + i]) and values_cap
 * as bpm_derive's.  bpm_pointwise_layout: out[4] = T (data per tile, threads per workgroup) | R (rows per staged tile) | row parts | rows per
 * part (the last part: what is left) of a launch over n_rows rows of d coordinates and n_data data -- a function of these numbers alone, not of
 * the device, the free memory or the environment.  Every partial result is merged in a fixed order (a thread's rows ascending, the parts in
 * index order) and there is no atomic: the bits are a function of (window, data, params).  An infinite or NaN l is counted and never reaches an
 * exp: no inf - inf is formed.  bipymc_amd/pointwise.py merges the ranks by the same formulas and finishes lppd, p_waic and elpd.
 * Nothing the samplers read is written (a history kept in position order is put into chain order first, as bpm_get_history does).  Errors: w
 * or n_data out of range, a source that does not compile (the compiler's log in bpm_last_error), no function installed, n_burn < 0, no
 * resident history (keep_history = 0), values beyond values_cap or of 2^31 elements or more, data, records or values larger than the free
 * device memory (the message names the requirement). */
int bpm_check_pointwise(const char* hip_source, int32_t w, const char* arch, char* log, int64_t log_cap);
int bpm_set_pointwise(bpm_handle_t h, const char* hip_source, const double* params, int32_t n_params, const double* data, int64_t n_data, int32_t w,
                      int32_t* reused);
int bpm_pointwise(bpm_handle_t h, int64_t n_burn, double* records, int64_t* n_rows, int64_t* n_first, double* values, int64_t values_cap);
int bpm_pointwise_layout(int32_t d, int32_t w, int64_t n_rows, int64_t n_data, int64_t* out);
/* PSIS-LOO PER DATUM (Vehtari, Simpson, Gelman, Yao and Gabry; Vehtari, Gelman and Gabry 2017) of the installed pointwise function, single rank.
 * With S the rows of the window and l the S values of a datum: M = ceil(min(S / 5, 3 sqrt(S / r_eff))), the kept set is the K = min(M + 1, S)
 * smallest l (bpm_loo_kept: K, or -1 for a bad argument), the cutoff c its largest, the tail the kept values < c.  Three stages per batch of
 * data (bipymc_amd/csrc/pointwise_tail.h, psis.h): A, compiled around the caller's source at the first call, selects every datum's kept set
 * exactly while the rows stream by (candidate columns in global scratch, a radix select when one fills); the library's segmented sort orders
 * it; B streams once more for the log-sum-exp of -l over the rows with l >= c, on bpm_pointwise_layout's fixed layout; C fits the generalised
 * Pareto distribution (Zhang and Stephens), smooths the tail and finishes, a workgroup per datum, every sum in a fixed order.
 * bpm_loo: r_eff[n_data] (finite, > 0); records = [8][n_data], field f of datum i at records[f * n_data + i]: 0 elpd_loo_i | 1 pareto_k (+inf
 * for a tail of 4 or fewer) | 2 sigma | 3 tail_len | 4 the kept values | 5 the body's rows (64-bit words) | 6, 7 (m, s): the body's
 * log-sum-exp of -l is m + log s.  A datum with a value that is not finite has NaN in 0, 1, 2 and 0 in 3.  tails (may be NULL):
 * tails[i * k_max + j], j < kept, ascending, at most tails_cap doubles, k_max = stats[1].  stats[12]: rows | k_max | stage A's row parts | data
 * batches | the most compactions one workgroup of stage A made | stage B's parts | its rows per part | the scratch budget in bytes | the
 * microseconds stages A (with the merge and the sort), B and C took on the device, summed over the batches | 1 if this call compiled the
 * module of stages A and B, 0 if the handle had kept it.
 * Selection is exact, so stage A's layout may depend on the budget: BPM_LOO_SCRATCH_MB, by default a quarter of the free device memory (read
 * at every call); the bits of every result do not depend on it.  bpm_loo_layout: out[8] = T | R | stage A's parts | its rows per part | tiles
 * per data batch | batches | stage B's parts | its rows per part for kept sets of k_max under a budget of budget_bytes.
 * Errors: what bpm_pointwise refuses, more than one rank, an r_eff that is not finite and > 0, tails beyond tails_cap, and kept sets of which
 * not even one tile of data fits the budget (refused before bpm_loo compiles or allocates anything -- the function bpm_set_pointwise
 * installed stays --; the message names the requirement), or whose one tile exceeds the sort's 2^31 keys. */
int64_t bpm_loo_kept(int64_t n_rows, double r_eff);
int bpm_loo_layout(int32_t d, int32_t w, int64_t n_rows, int64_t n_data, int64_t k_max, int64_t budget_bytes, int64_t* out);
int bpm_loo(bpm_handle_t h, int64_t n_burn, const double* r_eff, double* records, double* tails, int64_t tails_cap, int64_t* stats);
/* A DERIVED HISTORY IS A HISTORY: the installed function of `src` (bpm_set_device_function) over EVERY resident row of src, written into the
 * history of `dst` -- a second, ordinary handle made by bpm_create with the host-callback target, keep_history = 1, dim = n_out and src's
 * n_chains -- so that every statistic above (bpm_reduce_moments, bpm_diag_*, bpm_quantile_*, bpm_reduce_cov, bpm_hist_*, bpm_trace_*, bpm_derive
 * itself) answers about the derived quantities through dst, unchanged: the quantile band of a predicted curve, R-hat and ESS of the ratio
 * c_0 / c_inf one reports (what the reference computes on the host from param_est(n_burn)[2], examples/ex_exp_fit.py:176-202, and np.quantile
 * would add).  dst's row g, chain i, column m = output m of derive on src's row g, chain i (the padding column of an odd n_out is 0); dst's
 * ln-like history is src's; dst's state is its last row and its ln-like cache src's last ln-like row, what bpm_set_history and bpm_set_loglike
 * leave behind.  A snapshot: dst keeps describing src's history as it was at the call.  Nothing src's sampler reads is written (a history kept
 * in position order is put into chain order first, as bpm_get_history does): a run that continues is bit-identical to one that never made
 * the call.  Costs hist_rows x n_local x ((n_out rounded up to even) + 1) x 8 bytes of device memory on dst.  Every check runs before any
 * launch.  Errors: a null handle, dst == src, different devices, no function installed, no resident history on src (keep_history = 0), a dst
 * without keep_history, with another target, dim != n_out or another n_chains, world_size != 1 on either (single rank only), a derived history
 * larger than the free device memory (the message names the requirement).  A THINNED source (bpm_set_history_thin) gives an ordinary
 * stride-1 destination that holds the source's stored rows. */
int bpm_derive_history(bpm_handle_t src, bpm_handle_t dst);
/* A RANKED HISTORY IS A HISTORY: the one transform of a history that is no function of one sample -- the pooled rank of every value within
 * its coordinate -- written into the history of `dst`, a second, ordinary handle as bpm_derive_history takes one (host-callback target,
 * keep_history = 1, src's dim and n_chains), so that bpm_diag_split_moments / bpm_diag_autocov over dst give the rank-normalized split-R-hat
 * and the bulk and tail ESS of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), which Stan and ArviZ report (the reference stops at
 * param_est's mean and standard deviation); bipymc_amd/rank_diagnostics.py drives the fills.
 * The window is bpm_diag_split_moments': history rows [g_lo, g_hi), n = (g_hi - g_lo) / 2 (at least 4).  dst gets 2n rows: src's rows
 * [g_lo, g_lo + n), then [g_hi - n, g_hi) (an odd window drops its middle row), so the split statistics over dst's rows [0, 2n) use exactly
 * src's half-chains.  Per coordinate k over the S = 2 n n_local values of these rows, kind
 *   0  the average rank r (1-based; ties share the mean of their ranks; -0.0 and +0.0 are ties): half-integers, exact;
 *   1  z = Phi^-1((r - 3/8) / (S + 1/4)) of x;
 *   2  the same z of |x - arg[k]|;     4  the same r of |x - arg[k]|;
 *   3  1.0 where x <= arg[k], else 0.0 (no sort; n_pos must be 0).
 * arg: dim doubles (kinds 2, 3, 4; otherwise not read, may be NULL).  A coordinate whose window holds a NaN is NaN throughout (all kinds but
 * 3); +-inf are ordinary values.  order_stats[j * dim + k], j < n_pos (of |x - arg[k]| for kinds 2 and 4): the pos[j]-th smallest value
 * (0-based, pos[j] < S; NaN sorts last, so position S - 1 tells whether there is one; a zero comes back as +0.0) -- what a median and
 * np.quantile's interpolation need.  dst's ln-like history is src's rows of the same generations, its state its last row: dst comes out as
 * bpm_set_history and bpm_set_loglike leave a handle, and may be filled again.  A snapshot.  The columns are sorted in batches (one segment
 * of a segmented radix sort per column) of as many columns as fit a scratch budget -- keys in, keys out and the sort's temporaries, about
 * 24 S bytes per column; a quarter of the free memory; BPM_RANK_SCRATCH_MB in the environment sets it, BPM_RANK_BATCH_COLS the batch itself
 * -- and batch * S < 2^31; the result does not depend on the batch, the time does: the sort runs one workgroup per column.  Every check and every allocation comes before any launch;
 * nothing src's sampler reads is written (a history kept in position order is put into chain order first, as bpm_get_history does); every
 * temporary is freed on return.  Errors: a null handle, dst == src, different devices, an unknown kind, a missing arg, a position outside
 * [0, S), no resident history on src (keep_history = 0), a range out of bounds, n < 4, a dst without keep_history, with another target, dim
 * or n_chains, world_size != 1 on either (single rank only), S >= 2^31, one column's scratch beyond the budget or scratch or history beyond
 * the free device memory (the message names the requirement).  A THINNED source (bpm_set_history_thin): g_lo, g_hi count its stored rows and
 * dst is an ordinary stride-1 history of them. */
int bpm_rank_history(bpm_handle_t src, bpm_handle_t dst, int64_t g_lo, int64_t g_hi, int32_t kind, const double* arg, int32_t n_pos,
                     const int64_t* pos, double* order_stats);
/* kind 5 of bpm_rank_history, the squared deviation: dst[e * ld + k] = (x - arg[k]) * (x - arg[k]) over the same split rows -- the two IEEE
 * operations of NumPy's (x - c) ** 2, a flat fill without a sort like kind 3 (arg is needed, n_pos must be 0, the padding column of an odd
 * dim is 0).  With arg = the window's mean, the classic ESS over dst is the ESS of the variance estimate: what the Monte Carlo standard error
 * of a posterior standard deviation needs (bipymc_amd/summary.py). */
/* THE HIGHEST-DENSITY INTERVAL of every coordinate: the shortest interval that holds a share p of the window's draws -- what Stan's, ArviZ's
 * and the `posterior` package's summary tables print next to mean and sd (the reference stops at param_est's mean and standard deviation).
 * Definition, per coordinate k over the S values of the window and per probability p = prob[j], 0 < p < 1:
 *   s = the values sorted (NaN last; -0.0 and +0.0 are one value, +0.0);  m = min(floor(p * S), S - 1) in double arithmetic;
 *   w[i] = s[i + m] - s[i], i in [0, S - m);  i* = the first i whose w[i] is NaN (inf - inf) if there is one, else the first i of the
 *   smallest w (np.argmin's rule);  lo[j * dim + k] = s[i*], hi[j * dim + k] = s[i* + m].
 * A coordinate whose window holds a NaN has lo = hi = NaN; n_nan[k] counts its NaNs.  *count = S.
 * The window: window = 0, the split rows of history rows [a, b) -- n = (b - a) / 2 rows from a, then n rows up to b, S = 2 n n_local:
 * bpm_rank_history's and bpm_diag_split_moments' draws (n >= 1 here); window = 1, the super-chain rows >= a (b is not read), a partial
 * first generation counted by chain index: bpm_reduce_moments' selection, param_est(n_burn = a)'s rows.
 * order_stats[j * dim + k], j < n_pos: the pos[j]-th smallest value (0-based, pos[j] < S), from the same sorted columns, as
 * bpm_rank_history returns them (n_pos = 0: pos and order_stats are not read).
 * The columns are sorted in bpm_rank_history's batches under its scratch budget (BPM_RANK_SCRATCH_MB, BPM_RANK_BATCH_COLS); one scan of a
 * sorted column per probability.  The result depends neither on the batch nor on the launch shape: candidates are ordered by (width is NaN,
 * width, index), a total order, and no atomics are used.  Every check and every allocation comes before any launch; s's history is only
 * read (a history kept in position order is put into chain order first, as bpm_get_history does); every temporary is freed on return.
 * Errors: a null handle or output, an unknown window, n_prob outside 1 ... 8, a probability outside (0, 1), a position outside [0, S), no
 * resident history (keep_history = 0), a range out of bounds, an empty window, world_size != 1 (single rank only), S >= 2^31, one column's
 * scratch beyond the budget or scratch beyond the free device memory (the message names the requirement).  A THINNED history: a, b count
 * its stored rows. */
int bpm_hdi(bpm_handle_t s, int32_t window, int64_t a, int64_t b, int32_t n_prob, const double* prob, int32_t n_pos, const int64_t* pos,
            double* lo, double* hi, int64_t* n_nan, double* order_stats, int64_t* count);
/* (the test surface -- bpm_debug_*, bpm_selftest_philox, bpm_set_trace / bpm_get_trace, bpm_local_group_step, bpm_step_profiled, the
 * BPM_TEST_PATHS kernel-path switches -- is NOT part of this library: it is compiled only into build_variants/libbipymc_test.so and declared
 * in include/bipymc_hip_test.h; the product's kernel-argument block has no trace fields) */

#ifdef __cplusplus
}
#endif
#endif /* BIPYMC_HIP_H */
