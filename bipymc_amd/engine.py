"""Thin object wrapper over the C ABI: one `HipEngine` = one `bpm_handle_t`.

Mirrors, call for call, what DeMcMpi/DreamMpi need from the device: construction
(demc.py:14-32, dream.py:17-30), chain initialisation (chain.py:25-27), the
generation loop (demc.py:63-151), history (chain.py:51-54) and statistics.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


_dp_type = C.POINTER(C.c_double)
_ip_type = C.POINTER(C.c_int32)


class DeviceRows(object):
    """n rows of dim float64 coordinates in DEVICE memory (row stride ld doubles), read-only: what a device-resident likelihood is handed.  Exposes
    the CUDA array interface, which PyTorch-ROCm and CuPy-ROCm consume without a copy: `torch.as_tensor(rows, device="cuda")`."""

    def __init__(self, ptr, n, dim, ld, ids_ptr):
        self.ptr, self.n, self.dim, self.ld, self._ids_ptr = int(ptr), int(n), int(dim), int(ld), int(ids_ptr)
        self.shape = (self.n, self.dim)

    @property
    def __cuda_array_interface__(self):
        # (read-only by contract; PyTorch refuses the interface's read-only flag, so it is not set)
        return dict(shape=(self.n, self.dim), typestr="<f8", data=(self.ptr, False), strides=(self.ld * 8, 8), version=3)

    @property
    def ids(self):
        return _DeviceVector(self._ids_ptr, self.n, "<i4")

    def __len__(self):
        return self.n


class _DeviceVector(object):
    def __init__(self, ptr, n, typestr):
        self.ptr, self.n, self.typestr = int(ptr), int(n), typestr

    @property
    def __cuda_array_interface__(self):
        return dict(shape=(self.n,), typestr=self.typestr, data=(self.ptr, False), strides=None, version=3)


def _device_pointer(obj, n, what):
    """device address of a contiguous float64 vector of n values: anything with `__cuda_array_interface__` (torch / cupy arrays) or data_ptr()"""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if cai is not None:
        shape = tuple(cai["shape"])
        size = int(np.prod(shape)) if shape else 1
        if cai["typestr"] not in ("<f8", "=f8", "|f8"):
            raise TypeError("%s must be float64 on the device (got %s)" % (what, cai["typestr"]))
        if cai.get("strides") is not None and len(shape) == 1 and tuple(cai["strides"]) != (8,):
            raise ValueError("%s must be contiguous" % what)
        if len(shape) > 1 and size != max(shape):
            raise ValueError("%s must be one value per row (got shape %s)" % (what, shape))
        if n is not None and size != n:
            raise ValueError("%s: %d values for %d rows" % (what, size, n))
        return int(cai["data"][0])
    if hasattr(obj, "data_ptr"):
        return int(obj.data_ptr())
    raise TypeError("%s must live in device memory: an object with __cuda_array_interface__ (torch.Tensor on the GPU, cupy.ndarray)" % what)


class HipEngine(object):
    def __init__(self, algo, n_chains, dim, target_id, target_params, seed, device=0, rank=0, world_size=1,
                 nccl_uid=None, gamma_scale=1.0, del_pairs=3, burnin_gen=300, n_cr_gen=50, n_cr=3,
                 p_snooker=0.0, outlier_every=0, keep_history=True, running_moments=False, lib=None, thin=1):
        """thin: the history's stride (bpm_set_history_thin; 1 = a row per generation).  lib: the ctypes library to run on -- default the product library; tests that need the hooks of include/bipymc_hip_test.h pass
        `_lib.load_test()` (the same sources built with -DBPM_TEST_HOOKS)."""
        self._h = C.c_void_p()
        self.lib = lib if lib is not None else L.load()
        self.n_chains, self.dim = int(n_chains), int(dim)
        self.rank, self.world_size, self.device = int(rank), int(world_size), int(device)
        if self.n_chains % self.world_size != 0:
            raise ValueError("n_chains must be divisible by the communicator size")
        self.n_local = self.n_chains // self.world_size
        self.lo = self.rank * self.n_local
        tp = np.ascontiguousarray(target_params if target_params is not None else [], dtype=np.float64)
        cfg = L.BpmConfig()
        cfg.abi_version = L.ABI_VERSION
        cfg.algo = int(algo)
        cfg.n_chains = self.n_chains
        cfg.dim = self.dim
        cfg.target_id = int(target_id)
        cfg.n_target_params = int(tp.size)
        cfg.target_params = _dptr(tp) if tp.size else None
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.device = int(device)
        cfg.rank = self.rank
        cfg.world_size = self.world_size
        cfg.nccl_uid = bytes(nccl_uid) if nccl_uid is not None else None
        cfg.gamma_scale = float(gamma_scale)
        cfg.del_pairs = int(del_pairs)
        cfg.burnin_gen = int(burnin_gen)
        cfg.n_cr_gen = int(n_cr_gen)
        cfg.n_cr = int(n_cr)
        cfg.p_snooker = float(p_snooker)
        cfg.outlier_every = int(outlier_every)
        cfg.keep_history = 1 if keep_history else 0
        cfg.running_moments = 1 if running_moments else 0
        self._ck(self.lib.bpm_create(C.byref(cfg), C.byref(self._h)))
        if int(thin) != 1:
            try:
                self.set_history_thin(thin)
            except BaseException:
                self.close()
                raise
        self.algo, self.target_id = int(algo), int(target_id)
        self.n_cr = int(n_cr) if algo == L.ALGO_DREAM else 1

    def _ck(self, rc):
        L.check(rc, self.lib)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(L.UID_BYTES)
        L.check(L.load().bpm_get_unique_id(buf))
        return buf.raw

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            h, self._h = self._h, C.c_void_p()
            self._ck(self.lib.bpm_destroy(h))         # non-zero: the queue failed and buffers were leaked (include/bipymc_hip.h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ------------------------------------------------------
    def init_chains(self, theta_0, varepsilon):
        t0 = np.ascontiguousarray(np.asarray(theta_0, dtype=np.float64).reshape(-1))
        if t0.size != self.dim:
            raise ValueError("theta_0 has %d entries, dim is %d" % (t0.size, self.dim))
        var = np.ascontiguousarray(np.broadcast_to(np.asarray(varepsilon, dtype=np.float64), (self.dim,)))
        self._ck(self.lib.bpm_init_chains(self._h, _dptr(t0), _dptr(var)))

    def set_state(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.shape != (self.n_chains, self.dim):
            raise ValueError("state must have shape (n_chains, dim)")
        self._ck(self.lib.bpm_set_state(self._h, _dptr(X)))

    def get_state(self):
        X = np.empty((self.n_chains, self.dim), dtype=np.float64)
        self._ck(self.lib.bpm_get_state(self._h, _dptr(X)))
        return X

    def set_history(self, hist_local, X, thin=1, rows_logical=None):
        """Warm start.  thin = 1: a row per generation, X the last row of every chain (bpm_set_history).  thin = k > 1 or a rows_logical: the rows
        of a thinned history -- logical rows 0, k, 2k, ... of rows_logical (default: the last stored row is the last generation) -- and X the
        CURRENT state, which is the last row only when (rows_logical - 1) % k == 0 (bpm_set_history_thinned)."""
        hist_local = np.ascontiguousarray(hist_local, dtype=np.float64)
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert hist_local.ndim == 3 and hist_local.shape[1:] == (self.n_local, self.dim)
        assert X.shape == (self.n_chains, self.dim)
        if int(thin) == 1 and rows_logical is None:
            self._ck(self.lib.bpm_set_history(self._h, hist_local.shape[0], _dptr(hist_local), _dptr(X)))
            return
        if rows_logical is None:
            rows_logical = (hist_local.shape[0] - 1) * int(thin) + 1
        self._ck(self.lib.bpm_set_history_thinned(self._h, hist_local.shape[0], _dptr(hist_local), _dptr(X), int(thin), int(rows_logical)))

    # ---- thinned histories (include/bipymc_hip.h: bpm_set_history_thin) ---------------------------------
    def set_history_thin(self, k):
        """record every k-th generation from now on; only while the history holds its initial row"""
        self._ck(self.lib.bpm_set_history_thin(self._h, int(k)))

    def history_thin(self):
        """-> dict(thin, rows_logical, rows, last_stored): the stride, 1 + generations since (re)initialisation, the stored rows and the logical
        index of the last stored row (bpm_get_history_thin)"""
        out = (C.c_int64 * 4)()
        self._ck(self.lib.bpm_get_history_thin(self._h, out))
        return dict(thin=int(out[0]), rows_logical=int(out[1]), rows=int(out[2]), last_stored=int(out[3]))

    def thin_history(self, m):
        """keep stored rows 0, m, 2m, ...: the stride grows m-fold and the memory of the dropped rows is returned (bpm_thin_history)"""
        self._ck(self.lib.bpm_thin_history(self._h, int(m)))

    def debug_welford(self):
        """-> (mean, m2), (n_local, dim) each: the Welford records of DREAM's CR statistic.  Test variant only."""
        self._need_hooks("bpm_debug_get_welford")
        ld = self.dim + (self.dim & 1)
        mean = np.empty((self.n_local, ld)); m2 = np.empty((self.n_local, ld))
        self._ck(self.lib.bpm_debug_get_welford(self._h, _dptr(mean), _dptr(m2)))
        return mean[:, :self.dim].copy(), m2[:, :self.dim].copy()

    def set_loglike(self, ll_local):
        ll = np.ascontiguousarray(ll_local, dtype=np.float64)
        assert ll.shape == (self.n_local,)
        self._ck(self.lib.bpm_set_loglike(self._h, _dptr(ll)))

    def get_loglike(self):
        ll = np.empty(self.n_local, dtype=np.float64)
        self._ck(self.lib.bpm_get_loglike(self._h, _dptr(ll)))
        return ll

    # ---- running ----------------------------------------------------
    def begin_run(self, flip=0.5, shuffle=True, epsilon=None, u_epsilon=None, gamma=None):
        o = L.BpmRunOpts()
        o.flip = float(flip)
        o.shuffle = 1 if shuffle else 0
        o.epsilon = -1.0 if epsilon is None else float(epsilon)
        o.u_epsilon = -1.0 if u_epsilon is None else float(u_epsilon)
        o.gamma = -1.0 if gamma is None else float(gamma)
        self._ck(self.lib.bpm_begin_run(self._h, C.byref(o)))

    def step(self, n_gens):
        self._ck(self.lib.bpm_step(self._h, int(n_gens)))

    def step_timed(self, n_gens, read=True):
        """n_gens generations, synchronous, timed on the device -> (ms from the end of the first update launch to the end of the
        last, launches in that interval).  read=False returns nothing: fetch the figures with last_step_time() afterwards (reading
        the events costs tens of microseconds of host time)."""
        if not read:
            self._ck(self.lib.bpm_step_timed(self._h, int(n_gens), None, None))
            return None
        ms = C.c_float(0.0)
        n = C.c_int64(0)
        self._ck(self.lib.bpm_step_timed(self._h, int(n_gens), C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def last_step_time(self):
        ms = C.c_float(0.0)
        n = C.c_int64(0)
        self._ck(self.lib.bpm_get_step_time(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def _need_hooks(self, name):
        if not hasattr(self.lib, name):
            raise L.BpmError("%s is part of the test surface (include/bipymc_hip_test.h): create the engine with lib=_lib.load_test()" % name)

    def step_profiled(self, n_gens):
        """-> (summed update-kernel time in ms, number of launches).  Test variant only."""
        self._need_hooks("bpm_step_profiled")
        ms = C.c_double(0.0)
        n = C.c_int64(0)
        self._ck(self.lib.bpm_step_profiled(self._h, int(n_gens), C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def synchronize(self):
        self._ck(self.lib.bpm_synchronize(self._h))

    def propose(self, fresh=False):
        """-> (proposals (n, dim), global chain ids (n,)) of this rank's chains of the open half generation.  The arrays are views of two buffers the
        engine keeps (a fresh 3 MB NumPy array per half generation is 800 page faults under the library's copy: a fifth of the call at cfg2's shape):
        valid until the next propose(); fresh=True returns arrays of the caller's own."""
        if fresh or getattr(self, "_prop_host", None) is None:
            prop = np.empty((self.n_local, self.dim), dtype=np.float64)
            ids = np.empty(self.n_local, dtype=np.int32)
            if not fresh:
                self._prop_host, self._ids_host = prop, ids
        else:
            prop, ids = self._prop_host, self._ids_host
        n = C.c_int32(0)
        self._ck(self.lib.bpm_propose(self._h, _dptr(prop), _iptr(ids), C.byref(n)))
        return prop[:n.value], ids[:n.value]

    def commit(self, ll_prop):
        ll = np.ascontiguousarray(ll_prop, dtype=np.float64)
        self._ck(self.lib.bpm_commit(self._h, _dptr(ll) if ll.size else None))

    # ---- the same half generation, read-back overlapped with the caller's evaluation (bpm_propose_begin / _chunk, bpm_commit_chunk / _end) --------
    def propose_chunks(self, n_chunks):
        """Generator over the half generation's proposals in n_chunks pieces: yields (k, rows, ids) with rows an (n, dim) float64 VIEW into the
        library's pinned staging (valid until commit_end) and ids the global chain ids (-1 = idle work item); while the caller evaluates piece k
        the DMA of the following pieces proceeds.  Hand the values in with commit_chunk(k, ll) and finish with commit_end()."""
        self._ck(self.lib.bpm_propose_begin(self._h, int(n_chunks)))
        for k in range(int(n_chunks)):
            rows, ids = _dp_type(), _ip_type()
            n, ld = C.c_int32(0), C.c_int32(0)
            self._ck(self.lib.bpm_propose_chunk(self._h, k, C.byref(rows), C.byref(ids), C.byref(n), C.byref(ld)))
            if n.value == 0:
                yield k, np.empty((0, self.dim)), np.empty(0, dtype=np.int32)
                continue
            a = np.ctypeslib.as_array(rows, shape=(n.value, ld.value))[:, :self.dim]
            yield k, a, np.ctypeslib.as_array(ids, shape=(n.value,))

    def propose_begin(self, n_chunks):
        self._ck(self.lib.bpm_propose_begin(self._h, int(n_chunks)))

    def propose_chunk(self, k):
        """piece k of the open half generation (waits for its DMA only; callable from a worker thread) -> (rows view, ids view)"""
        rows, ids = _dp_type(), _ip_type()
        n, ld = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.bpm_propose_chunk(self._h, int(k), C.byref(rows), C.byref(ids), C.byref(n), C.byref(ld)))
        if n.value == 0:
            return np.empty((0, self.dim)), np.empty(0, dtype=np.int32)
        return np.ctypeslib.as_array(rows, shape=(n.value, ld.value))[:, :self.dim], np.ctypeslib.as_array(ids, shape=(n.value,))

    def commit_chunk(self, k, ll):
        ll = np.ascontiguousarray(ll, dtype=np.float64)
        self._ck(self.lib.bpm_commit_chunk(self._h, int(k), _dptr(ll) if ll.size else None))

    def commit_end(self):
        self._ck(self.lib.bpm_commit_end(self._h))

    # ---- ... and with the likelihood evaluated on the device by the caller's framework (bpm_propose_device / bpm_commit_device) --------------------
    def propose_device(self):
        """-> DeviceRows: the half generation's proposals where they lie in device memory (`__cuda_array_interface__`: torch.as_tensor / cupy.asarray
        take it without a copy), work-item order; .ids is the same for the global chain ids (-1 = idle work item)"""
        rows, ids = C.c_void_p(), C.c_void_p()
        n, ld = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.bpm_propose_device(self._h, C.byref(rows), C.byref(ids), C.byref(n), C.byref(ld)))
        return DeviceRows(rows.value or 0, n.value, self.dim, ld.value, ids.value or 0)

    def commit_device(self, ll):
        """ll: n float64 values in device memory, in the order of the rows (anything with `__cuda_array_interface__` or data_ptr())"""
        self._ck(self.lib.bpm_commit_device(self._h, C.c_void_p(_device_pointer(ll, self._pending_rows(), "ln_like values"))))

    def _pending_rows(self):
        return None

    def state_device(self):
        rows = C.c_void_p()
        n, ld = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.bpm_state_device(self._h, C.byref(rows), C.byref(n), C.byref(ld)))
        return DeviceRows(rows.value or 0, n.value, self.dim, ld.value, 0)

    def set_loglike_device(self, ll):
        self._ck(self.lib.bpm_set_loglike_device(self._h, C.c_void_p(_device_pointer(ll, self.n_local, "ln_like values"))))

    def set_device_likelihood(self, source, params=(), data=None):
        """ln_like_fn as HIP source (include/bipymc_hip.h: bpm_set_device_likelihood): compiled with hiprtc into a kernel that runs between the proposal
        and the commit kernel; `step` then drives this host-callback sampler.  The current states are evaluated at once.
        data (n_data, w) float64: the per-datum form (bpm_set_device_likelihood_data) -- copied to the device once, summed a wavefront per chunk."""
        p = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        src = source.encode() if isinstance(source, str) else bytes(source)
        pp = p.ctypes.data_as(C.POINTER(C.c_double)) if p.size else None
        if data is None:
            self._ck(self.lib.bpm_set_device_likelihood(self._h, src, pp, int(p.size)))
        else:
            dat = np.asarray(data)
            if dat.dtype != np.float64 or dat.ndim not in (1, 2) or dat.size == 0:
                raise ValueError("data must be a non-empty float64 array of shape (n_data, w) or (n_data,)")
            dat = np.ascontiguousarray(dat.reshape(dat.shape[0], -1))
            self._ck(self.lib.bpm_set_device_likelihood_data(self._h, src, pp, int(p.size), _dptr(dat), dat.shape[0], dat.shape[1]))
        self.has_device_likelihood = True

    def eval_device_likelihood(self, X):
        """the installed device likelihood (any form) at the rows of X (n, dim), by its kernel of its own (bpm_eval_device_likelihood)"""
        X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
        if X.shape[1] != self.dim:
            raise ValueError("X must have %d columns (got %d)" % (self.dim, X.shape[1]))
        out = np.empty(X.shape[0], dtype=np.float64)
        self._ck(self.lib.bpm_eval_device_likelihood(self._h, _dptr(X), X.shape[0], _dptr(out)))
        return out

    @staticmethod
    def data_likelihood_chunk():
        """consecutive data points one wavefront sums in the per-datum form (bpm_data_likelihood_chunk)"""
        return int(L.load().bpm_data_likelihood_chunk())

    def device_likelihood_info(self):
        """-> (fused, why): fused True -- the update kernel itself was compiled around the likelihood (one launch per half generation); False -- the
        proposal / likelihood / commit kernels run, `why` says why the fused form is not in use"""
        fused = C.c_int32(0)
        why = C.create_string_buffer(1 << 14)
        self._ck(self.lib.bpm_get_device_likelihood_info(self._h, C.byref(fused), why, len(why)))
        return bool(fused.value), why.value.decode(errors="replace")

    def refresh_device_loglike(self):
        self._ck(self.lib.bpm_refresh_device_loglike(self._h))

    def reserve_history(self, rows):
        self._ck(self.lib.bpm_reserve_history(self._h, int(rows)))

    # ---- results ----------------------------------------------------
    def stats(self):
        st = L.BpmStats()
        self._ck(self.lib.bpm_get_stats(self._h, C.byref(st)))
        n = st.n_cr
        return dict(local_n_accepted=st.local_n_accepted, local_n_rejected=st.local_n_rejected,
                    n_nan_alpha=st.n_nan_alpha, k_gen=st.k_gen, t_abs=st.t_abs, history_rows=st.history_rows,
                    n_outlier_resets=st.n_outlier_resets,
                    p_cr=np.array(st.p_cr[:n]), delta_m=np.array(st.delta_m[:n]),
                    n_cr_updates=np.array(st.n_cr_updates[:n]))

    EXCHANGE_MODES = {"dense": 0, "rows": 1, "replay": 2, "push": 3}

    def set_exchange(self, mode="replay", cap=0):
        """world_size > 1: "push" (owners store accepted rows straight into the peers' replicas; the default once connected),
        "replay" (accept bytes through RCCL + recomputation), "rows" (accepted rows in packed blocks; cap = rows per sub-block
        per half generation) or "dense" (all-gather of whole blocks)"""
        if mode == "push-agent":          # the push exchange with agent-scope packet fences (include/bipymc_hip.h: bpm_set_exchange)
            mode, cap = "push", 1
        self._ck(self.lib.bpm_set_exchange(self._h, self.EXCHANGE_MODES[mode], int(cap)))

    def exchange_stats(self):
        out = (C.c_int64 * 8)()
        self._ck(self.lib.bpm_get_exchange_stats(self._h, out))
        return dict(mode=["dense", "rows", "replay", "push"][out[0]], cap=int(out[1]), chunks=int(out[2]), replays=int(out[3]),
                    replay_gens=int(out[4]), push_gens=int(out[5]), push_connected=bool(int(out[6]) & 3), push_flags_fine_grained=(int(out[6]) & 3) == 2,
                    # bpm_push_selftest's arena probe: stores into the peers' arenas arrived under system- / agent-scope packet fences; run on the own queue
                    arena_probe_system=bool(int(out[6]) & 4), arena_probe_agent=bool(int(out[6]) & 8), arena_probe_on_own_queue=bool(int(out[6]) & 16),
                    barriers=int(out[7]) & ((1 << 62) - 1), push_fence_scope="agent" if int(out[7]) >> 62 & 1 else "system")

    # ---- push exchange (world_size > 1): map the ranks' buffers into each other ------------------------------------------
    def push_export(self):
        """-> bytes: what the other ranks need to map this rank's exchange buffer (bpm_push_export)"""
        buf = C.create_string_buffer(L.PUSH_BLOB_BYTES)
        self._ck(self.lib.bpm_push_export(self._h, buf))
        return buf.raw

    def push_connect(self, blobs):
        """blobs: the exports of ALL ranks in rank order (bpm_push_connect)"""
        blobs = [bytes(b) for b in blobs]
        if len(blobs) != self.world_size or any(len(b) != L.PUSH_BLOB_BYTES for b in blobs):
            raise ValueError("push_connect needs one export per rank")
        buf = C.create_string_buffer(b"".join(blobs), L.PUSH_BLOB_BYTES * self.world_size)
        self._ck(self.lib.bpm_push_connect(self._h, buf))

    def push_selftest(self):
        """collective over the ranks (one engine per process): -> True when this rank received every peer's pattern"""
        arr = (C.c_void_p * 1)(self._h)
        ok = C.c_int32(0)
        self._ck(self.lib.bpm_push_selftest(arr, 1, C.byref(ok)))
        return bool(ok.value)

    @staticmethod
    def push_uid():
        """the nccl_uid of a world WITHOUT an RCCL communicator: the push exchange is its only one"""
        return b"BPMPUSH" + bytes(L.UID_BYTES - 7)

    def launch_stats(self):
        """How the update kernels were dispatched: the library's own AQL queue or the HIP stream (bpm_get_launch_stats)."""
        out = (C.c_int64 * 6)()
        self._ck(self.lib.bpm_get_launch_stats(self._h, out))
        return dict(has_queue=bool(out[0]), direct=int(out[1]), stream=int(out[2]), queue_active=bool(out[3]),
                    coherent_state=bool(out[4]), fence={3: "acquire+release", 1: "acquire", 0: "none"}.get(int(out[5]), int(out[5])))

    def set_launch_path(self, direct=True, fence=-1):
        """direct=False: HIP stream launches only; fence: 3 acquire + release, 1 acquire only, 0 none, -1 keep (bpm_set_launch_path)."""
        self._ck(self.lib.bpm_set_launch_path(self._h, 1 if direct else 0, int(fence)))

    def history_rows(self):
        return int(self.stats()["history_rows"])

    def get_history(self, g_lo=0, g_hi=None):
        """(g_hi - g_lo, n_local, dim): row g, local chain i."""
        if g_hi is None:
            g_hi = self.history_rows()
        out = np.empty((max(0, g_hi - g_lo), self.n_local, self.dim), dtype=np.float64)
        self._ck(self.lib.bpm_get_history(self._h, int(g_lo), int(g_hi), _dptr(out)))
        return out

    def get_loglike_history(self, g_lo=0, g_hi=None):
        if g_hi is None:
            g_hi = self.history_rows()
        out = np.empty((max(0, g_hi - g_lo), self.n_local), dtype=np.float64)
        self._ck(self.lib.bpm_get_loglike_history(self._h, int(g_lo), int(g_hi), _dptr(out)))
        return out

    def reduce_moments(self, n_burn=0):
        """-> (count, S1, S2, shift): raw moments of the local super-chain rows >= n_burn."""
        s1 = np.empty(self.dim); s2 = np.empty(self.dim); sh = np.empty(self.dim)
        n = C.c_int64(0)
        self._ck(self.lib.bpm_reduce_moments(self._h, int(n_burn), _dptr(s1), _dptr(s2), _dptr(sh), C.byref(n)))
        return int(n.value), s1, s2, sh

    def diag_split_moments(self, g_lo, g_hi):
        """-> (mean_of_means, m2_of_means, sum_of_vars, n_half_chains, n_draws): split-chain moments of this rank's chains over history rows
        [g_lo, g_hi) (bpm_diag_split_moments; bipymc_amd/diagnostics.py finishes them)"""
        mm = np.empty(self.dim); m2 = np.empty(self.dim); sv = np.empty(self.dim)
        m = C.c_int64(0); n = C.c_int64(0)
        self._ck(self.lib.bpm_diag_split_moments(self._h, int(g_lo), int(g_hi), _dptr(mm), _dptr(m2), _dptr(sv), C.byref(m), C.byref(n)))
        return mm, m2, sv, int(m.value), int(n.value)

    def diag_autocov(self, t0, n_lags):
        """-> (n_lags, dim): sum over this rank's half-chains of the biased autocovariance at lags t0 ... t0 + n_lags - 1, on the window of the
        last diag_split_moments call"""
        out = np.empty((int(n_lags), self.dim))
        self._ck(self.lib.bpm_diag_autocov(self._h, int(t0), int(n_lags), _dptr(out)))
        return out

    def quantile_begin(self, n_burn):
        """-> this rank's number of super-chain rows >= n_burn (the window of the quantile_histogram calls that follow; bpm_quantile_begin)"""
        n = C.c_int64(0)
        self._ck(self.lib.bpm_quantile_begin(self._h, int(n_burn), C.byref(n)))
        return int(n.value)

    def quantile_histogram(self, prefix_dim, prefixes, bits):
        """-> (hist (n_prefix, 256) uint64, n_nan (n_prefix,) int64): this rank's keys of the window under each (coordinate, prefix) slot by
        their next 8 bits (bpm_quantile_histogram; bipymc_amd/quantiles.py runs the select)"""
        pk = np.ascontiguousarray(prefix_dim, dtype=np.int32)
        pv = np.ascontiguousarray(prefixes, dtype=np.uint64)
        hist = np.empty((len(pk), 256), dtype=np.uint64)
        nn = np.empty(len(pk), dtype=np.int64)
        self._ck(self.lib.bpm_quantile_histogram(self._h, len(pk), pk.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 pv.ctypes.data_as(C.POINTER(C.c_uint64)), int(bits),
                                                 hist.ctypes.data_as(C.POINTER(C.c_uint64)), nn.ctypes.data_as(C.POINTER(C.c_int64))))
        return hist, nn

    def reduce_cov(self, n_burn, center):
        """-> (count, S1 (dim,), S2 (dim, dim)): sum (x - center) and sum (x - center)(x - center)^T over the local super-chain rows >= n_burn
        (bpm_reduce_cov; bipymc_amd/covariance.py merges the ranks and finishes the covariance)"""
        c = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(self.dim)
        s1 = np.empty(self.dim); s2 = np.empty((self.dim, self.dim))
        n = C.c_int64(0)
        self._ck(self.lib.bpm_reduce_cov(self._h, int(n_burn), None if c is None else _dptr(c), _dptr(s1), _dptr(s2), C.byref(n)))
        return int(n.value), s1, s2

    def hist_range(self, n_burn):
        """-> (count, lo (dim,), hi (dim,), n_nan (dim,), n_inf (dim,)): over the local super-chain rows >= n_burn, the smallest and largest
        value of every coordinate that is not NaN (+inf / -inf where there is none) and how many are NaN / infinite; fixes the window of the
        hist_marginals / hist_pairs calls that follow (bpm_hist_range; bipymc_amd/histograms.py builds the edges and merges the ranks)"""
        lo = np.empty(self.dim); hi = np.empty(self.dim)
        nn = np.empty(self.dim, dtype=np.int64); ni = np.empty(self.dim, dtype=np.int64)
        n = C.c_int64(0)
        i64 = C.POINTER(C.c_int64)
        self._ck(self.lib.bpm_hist_range(self._h, int(n_burn), _dptr(lo), _dptr(hi), nn.ctypes.data_as(i64), ni.ctypes.data_as(i64), C.byref(n)))
        return int(n.value), lo, hi, nn, ni

    def hist_marginals(self, dims, edges):
        """-> (m, bins) int64: np.histogram's counts of the coordinates `dims` (m,) for the edges (m, bins + 1) over the window of the last
        hist_range call (bpm_hist_marginals)"""
        dm = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1)
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(len(dm), -1)
        out = np.empty((len(dm), e.shape[1] - 1), dtype=np.int64)
        self._ck(self.lib.bpm_hist_marginals(self._h, len(dm), dm.ctypes.data_as(C.POINTER(C.c_int32)), e.shape[1] - 1, _dptr(e),
                                             out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def hist_pairs(self, dims, edges2d, pair_a, pair_b):
        """-> (P, bins2d, bins2d) int64: np.histogram2d's counts of the pairs (dims[pair_a[p]], dims[pair_b[p]]) for the edges (m, bins2d + 1)
        over the window of the last hist_range call (bpm_hist_pairs)"""
        dm = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1)
        e = np.ascontiguousarray(edges2d, dtype=np.float64).reshape(len(dm), -1)
        pa = np.ascontiguousarray(pair_a, dtype=np.int32).reshape(-1)
        pb = np.ascontiguousarray(pair_b, dtype=np.int32).reshape(-1)
        nb = e.shape[1] - 1
        out = np.empty((len(pa), nb, nb), dtype=np.int64)
        i32 = C.POINTER(C.c_int32)
        self._ck(self.lib.bpm_hist_pairs(self._h, len(dm), dm.ctypes.data_as(i32), nb, _dptr(e), len(pa), pa.ctypes.data_as(i32),
                                         pb.ctypes.data_as(i32), out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def trace_bins(self, g_lo, g_hi, every):
        """-> (counts (2, T, dim) int64, sums (5, T, dim), ll_counts (4, T) int64, ll_sums (5, T), best_ll, best_row, best_x (dim,)): per bin of
        `every` history rows of [g_lo, g_hi) over this rank's chains, how many values are finite | NaN, and a shift | the shifted sum | the
        shifted sum of squares of the finite ones | min | max; the same over the ln-likes (counts: finite | NaN | +inf | -inf); the rank's
        largest ln-like, its row of the super chain g * n_chains + i (-1: none that is not NaN) and that row.  Fixes the bins of the
        trace_chains calls that follow (bpm_trace_bins; bipymc_amd/traces.py merges the ranks)"""
        g_lo, g_hi, every = int(g_lo), int(g_hi), int(every)
        span = max(0, g_hi - g_lo)
        T = -(-span // min(max(every, 1), max(span, 1)))         # (a bin wider than the range is the range)
        counts = np.zeros((2, T, self.dim), dtype=np.int64); sums = np.zeros((5, T, self.dim))
        ll_counts = np.zeros((4, T), dtype=np.int64); ll_sums = np.zeros((5, T))
        best_ll = C.c_double(0.0); best_row = C.c_int64(-1); best_x = np.empty(self.dim)
        i64 = C.POINTER(C.c_int64)
        self._ck(self.lib.bpm_trace_bins(self._h, g_lo, g_hi, every, counts.ctypes.data_as(i64), _dptr(sums), ll_counts.ctypes.data_as(i64),
                                         _dptr(ll_sums), C.byref(best_ll), C.byref(best_row), _dptr(best_x)))
        self._trace_T = T
        row = int(best_row.value)
        if row >= 0:
            row = (row // self.n_local) * self.n_chains + self.lo + row % self.n_local
        return counts, sums, ll_counts, ll_sums, float(best_ll.value), row, best_x

    def trace_chains(self, chains):
        """-> (pos (c,), x (T, c, dim), ll (T, c)): those of the global chains `chains` this rank holds (pos: their positions in `chains`) at
        the first history row of every bin of the last trace_bins call (bpm_trace_chains)"""
        ch = np.asarray(chains, dtype=np.int64).reshape(-1)
        pos = np.nonzero((ch >= self.lo) & (ch < self.lo + self.n_local))[0]
        if len(pos) == 0:
            return pos, np.empty((0, 0, self.dim)), np.empty((0, 0))
        ids = np.ascontiguousarray(ch[pos] - self.lo, dtype=np.int32)
        T = getattr(self, "_trace_T", 0)
        x = np.empty((T, len(ids), self.dim)); ll = np.empty((T, len(ids)))
        self._ck(self.lib.bpm_trace_chains(self._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(x), _dptr(ll)))
        return pos, x, ll

    def set_device_function(self, source, n_out, params=()):
        """A function of one sample as HIP source (include/bipymc_hip.h: bpm_set_device_function): compiled around the window reduction of
        bipymc_amd/csrc/derived.h and kept on the handle; the same source and n_out again only copy `params`"""
        p = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        src = source.encode() if isinstance(source, str) else bytes(source)
        self._ck(self.lib.bpm_set_device_function(self._h, src, int(n_out), _dptr(p) if p.size else None, int(p.size)))
        self._derive_n_out = int(n_out)

    def window_rows(self, n_burn):
        """this rank's rows of the window at or after n_burn >= 0 (super_chain_window's count: a partial first generation by chain index)"""
        G = self.history_rows()
        g0, first = n_burn // self.n_chains, min(max(n_burn % self.n_chains - self.lo, 0), self.n_local)
        return max(0, (G - g0) * self.n_local - first) if g0 < G else 0

    def _values_cap(self, who, n_burn, per_row, noun):
        """-> the elements of the `values` a statistic returns over that window, per_row of them a row (0 for a negative n_burn: the library
        refuses it); 2^31 or more are refused -- here, before anything is installed or allocated"""
        rows = self.window_rows(n_burn) if n_burn >= 0 else 0
        if rows * per_row >= 1 << 31:
            raise ValueError("%s: the values of %d rows x %d %s are %d elements; fewer than 2^31 per rank can be returned"
                             % (who, rows, per_row, noun, rows * per_row))
        return rows * per_row

    def derive_rows(self, n_burn, values=False):
        """-> (counts (2, n_out) int64, sums (5, n_out), n_rows, n_first, values (n_rows, n_out) or None): the installed function over this
        rank's super-chain rows >= n_burn -- per output how many values are finite | NaN, and a shift | the shifted sum | the shifted sum of
        squares of the finite ones | min | max; n_first of the n_rows rows lie in a partial first generation (bpm_derive)"""
        m = getattr(self, "_derive_n_out", 0)
        n_burn = int(n_burn)
        counts = np.zeros((2, max(m, 1)), dtype=np.int64); sums = np.zeros((5, max(m, 1)))
        n_rows = C.c_int64(0); n_first = C.c_int64(0)
        vals, cap = None, 0
        if values and m and n_burn >= 0:
            cap = self._values_cap("param_est_fn", n_burn, m, "outputs")
            vals = np.empty(max(cap, 1))
        i64 = C.POINTER(C.c_int64)
        self._ck(self.lib.bpm_derive(self._h, n_burn, counts.ctypes.data_as(i64), _dptr(sums), C.byref(n_rows), C.byref(n_first),
                                     None if vals is None else _dptr(vals), cap))
        n = int(n_rows.value)
        return counts[:, :m], sums[:, :m], n, int(n_first.value), None if vals is None else vals[:n * m].reshape(n, m)

    def derive(self, fn, n_burn, values=False):
        """derived.compute's per-rank call: installs `fn` (a derived.HipFunction) and reduces (set_device_function + derive_rows).  The
        values of 2^31 elements or more are refused before anything is installed or allocated."""
        if values:
            self._values_cap("param_est_fn", int(n_burn), fn.n_out, "outputs")
        self.set_device_function(fn.source, fn.n_out, fn.params)
        return self.derive_rows(n_burn, values)

    def set_pointwise(self, source, data, params=()):
        """The log density of one datum as HIP source (include/bipymc_hip.h: bpm_set_pointwise): compiled around the streaming reduction of
        bipymc_amd/csrc/pointwise_rows.h and kept on the handle with a device copy of `data` (n_data, w); the same source, w and data
        again only copy `params`.  -> True when the loaded program and the data were kept"""
        p = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        y = np.ascontiguousarray(data, dtype=np.float64)
        src = source.encode() if isinstance(source, str) else bytes(source)
        reused = C.c_int32(0)
        self._ck(self.lib.bpm_set_pointwise(self._h, src, _dptr(p) if p.size else None, int(p.size), _dptr(y), int(y.shape[0]), int(y.shape[1]),
                                            C.byref(reused)))
        self._pointwise_n_data = int(y.shape[0])
        return bool(reused.value)

    def pointwise_rows(self, n_burn, values=False):
        """-> (counts (4, n_data) int64, sums (5, n_data), n_rows, n_first, values (n_rows, n_data) or None): the installed pointwise
        function over this rank's super-chain rows >= n_burn -- per datum how many values are finite | NaN | +inf | -inf, and of the
        finite ones a shift | the shifted sum | the shifted sum of squares | their maximum m | s = sum exp(l - m); n_first of the n_rows
        rows lie in a partial first generation (bpm_pointwise)"""
        nd = getattr(self, "_pointwise_n_data", 0)
        n_burn = int(n_burn)
        rec = np.zeros((L.PW_FIELDS, max(nd, 1)))
        n_rows = C.c_int64(0); n_first = C.c_int64(0)
        vals, cap = None, 0
        if values and nd and n_burn >= 0:
            cap = self.window_rows(n_burn) * nd      # (called directly, 2^31 or more are the library's to refuse: pointwise() has refused them)
            vals = np.empty(max(cap, 1))
        self._ck(self.lib.bpm_pointwise(self._h, n_burn, _dptr(rec), C.byref(n_rows), C.byref(n_first), None if vals is None else _dptr(vals), cap))
        n = int(n_rows.value)
        rec = rec[:, :nd]
        counts = np.ascontiguousarray(rec[[L.PW_N, L.PW_NAN, L.PW_PINF, L.PW_NINF]]).view(np.int64)
        sums = np.ascontiguousarray(rec[[L.PW_C, L.PW_S1, L.PW_S2, L.PW_M, L.PW_S]])
        return counts, sums, n, int(n_first.value), None if vals is None else vals[:n * nd].reshape(n, nd)

    def pointwise(self, pw, n_burn, values=False):
        """pointwise.compute's per-rank call: installs `pw` (a pointwise.HipPointwise) and reduces (set_pointwise + pointwise_rows).  The
        values of 2^31 elements or more are refused before anything is installed or allocated."""
        if values:
            self._values_cap("param_est_waic", int(n_burn), pw.n_data, "data points")
        self.set_pointwise(pw.source, pw.data, pw.params)
        return self.pointwise_rows(n_burn, values)

    def pointwise_layout(self, n_rows, n_data, w=1):
        """-> (T, R, parts, rows per part): data per tile, rows per staged tile, row parts and the rows of a part (the last: what is left) of
        a launch over n_rows rows of this engine's dim and n_data data (bpm_pointwise_layout: a function of these numbers alone)"""
        out = (C.c_int64 * 4)()
        self._ck(self.lib.bpm_pointwise_layout(int(self.dim), int(w), int(n_rows), int(n_data), out))
        return tuple(int(x) for x in out)

    def loo_kept(self, n_rows, r_eff):
        """-> (n_data,) int64: the size K = min(ceil(min(S / 5, 3 sqrt(S / r_eff))) + 1, S) of each datum's kept set over a window of
        S = n_rows draws (bpm_loo_kept)"""
        return np.array([self.lib.bpm_loo_kept(int(n_rows), float(r)) for r in np.atleast_1d(r_eff)], dtype=np.int64)

    def loo_layout(self, n_rows, n_data, k_max, w=1, budget_bytes=1 << 62):
        """-> (T, R, stage A's row parts, its rows per part, tiles per data batch, data batches, stage B's parts, its rows per part) of
        bpm_loo over n_rows rows of this engine's dim, n_data data and kept sets of at most k_max values under a scratch budget
        (bpm_loo_layout; by default no budget to speak of: the layout the rows alone give)"""
        out = (C.c_int64 * 8)()
        self._ck(self.lib.bpm_loo_layout(int(self.dim), int(w), int(n_rows), int(n_data), int(k_max), int(budget_bytes), out))
        return tuple(int(x) for x in out)

    def loo(self, pw, n_burn, r_eff, tails=False):
        """pointwise.compute_loo's device call: installs `pw`, selects, fits and finishes (set_pointwise + bpm_loo).  r_eff: (n_data,).
        -> (records (LOO_FIELDS, n_data) float64 -- the count fields to be viewed as int64 --, stats dict, tails: None or a list of each
        datum's kept values, ascending)"""
        n_burn = int(n_burn)
        r = np.ascontiguousarray(r_eff, dtype=np.float64)
        nd = pw.n_data
        rows = self.window_rows(n_burn) if n_burn >= 0 else 0
        buf, cap = None, 0
        if tails and rows:
            k_max = int(self.loo_kept(rows, r.min()).max())
            cap = nd * k_max
            if cap >= 1 << 31:
                raise ValueError("param_est_loo: the tails of %d data x %d kept values are %d elements; fewer than 2^31 can be returned"
                                 % (nd, k_max, cap))
            buf = np.empty(max(cap, 1))
        self.set_pointwise(pw.source, pw.data, pw.params)
        rec = np.zeros((L.LOO_FIELDS, nd))
        stats = (C.c_int64 * 12)()
        self._ck(self.lib.bpm_loo(self._h, n_burn, _dptr(r), _dptr(rec), None if buf is None else _dptr(buf), cap, stats))
        names = ("rows", "k_max", "tail_parts", "batches", "compactions", "body_parts", "body_rows_per_part", "budget_bytes", "tail_us", "body_us", "fit_us", "compiled")
        st = dict(zip(names, (int(x) for x in stats)))
        out = None
        if buf is not None:
            kept = rec[L.LOO_KEPT].view(np.int64)
            out = [buf[i * st["k_max"]:i * st["k_max"] + int(kept[i])].copy() for i in range(nd)]
        elif tails:
            out = [np.empty(0) for _ in range(nd)]
        return rec, st, out

    def _second_engine(self, dim):
        """the destination of derive_history / rank_history: a history-keeping host-callback engine of this one's chains, library and device"""
        return HipEngine(algo=L.ALGO_DEMC, n_chains=self.n_chains, dim=dim, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=0,
                         device=self.device, burnin_gen=0, outlier_every=0, keep_history=True, lib=self.lib)

    def derive_history(self, fn):
        """-> HipEngine: a second, ordinary engine with dim = fn.n_out on the same library and device whose resident history is `fn` (a
        derived.HipFunction) of every row of this one's, with this one's log-likelihood history (bpm_derive_history) -- every statistic above
        then answers about the derived quantities through it.  A snapshot; the caller closes it.  Single rank only."""
        if self.world_size != 1:
            raise NotImplementedError("derive_history: a derived history is built on a single rank only (world_size = %d)" % self.world_size)
        self.set_device_function(fn.source, fn.n_out, fn.params)
        dst = self._second_engine(fn.n_out)
        try:
            self._ck(self.lib.bpm_derive_history(self._h, dst._h))
        except BaseException:
            dst.close()
            raise
        return dst

    def rank_history(self, g_lo, g_hi, kind, arg=None, positions=(), dst=None):
        """-> (HipEngine, order_stats (len(positions), dim)): a second, ordinary engine of this one's shape whose resident history is a
        transform of the split rows of history rows [g_lo, g_hi) -- kind 0 the pooled average ranks, 1 their normal scores, 2 those of
        |x - arg[k]|, 4 the ranks of |x - arg[k]|, 3 the indicator x <= arg[k], 5 the squared deviation (x - arg[k])^2 -- and the `positions`-th smallest values of every coordinate
        (bpm_rank_history; bipymc_amd/rank_diagnostics.py).  dst: an engine an earlier call returned, to be filled again (None: a new one,
        closed when the call fails).  A snapshot; the caller closes it.  Single rank only."""
        if self.world_size != 1:
            raise NotImplementedError("rank_history: pooled ranks are built on a single rank only (world_size = %d)" % self.world_size)
        a = None if arg is None else np.ascontiguousarray(np.asarray(arg, dtype=np.float64).reshape(self.dim))
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.int64).reshape(-1))
        out = np.empty((len(pos), self.dim), dtype=np.float64)
        own = dst is None
        if own:
            dst = self._second_engine(self.dim)
        try:
            self._ck(self.lib.bpm_rank_history(self._h, dst._h, int(g_lo), int(g_hi), int(kind), None if a is None else _dptr(a), len(pos),
                                               pos.ctypes.data_as(C.POINTER(C.c_int64)) if len(pos) else None, _dptr(out) if len(pos) else None))
        except BaseException:
            if own:
                dst.close()
            raise
        return dst, out

    def hdi(self, window, a, b, prob, positions=()):
        """-> (lo (len(prob), dim), hi (len(prob), dim), n_nan (dim,) int64, S, order_stats (len(positions), dim)): the highest-density
        intervals of every coordinate over `window` -- 0: the split rows of history rows [a, b) (rank_history's draws), 1: the super-chain rows
        >= a (param_est's) -- and the `positions`-th smallest values from the same sorted columns (bpm_hdi; bipymc_amd/summary.py).  Single
        rank only."""
        if self.world_size != 1:
            raise NotImplementedError("hdi: columns are sorted on a single rank only (world_size = %d)" % self.world_size)
        p = np.ascontiguousarray(np.asarray(prob, dtype=np.float64).reshape(-1))
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.int64).reshape(-1))
        lo = np.empty((len(p), self.dim)); hi = np.empty((len(p), self.dim))
        nn = np.empty(self.dim, dtype=np.int64)
        out = np.empty((len(pos), self.dim), dtype=np.float64)
        n = C.c_int64(0)
        i64 = C.POINTER(C.c_int64)
        self._ck(self.lib.bpm_hdi(self._h, int(window), int(a), int(b), len(p), _dptr(p) if len(p) else None, len(pos),
                                  pos.ctypes.data_as(i64) if len(pos) else None, _dptr(lo), _dptr(hi), nn.ctypes.data_as(i64),
                                  _dptr(out) if len(pos) else None, C.byref(n)))
        return lo, hi, nn, int(n.value), out

    def set_adapt_state(self, p_cr=None, delta_m=None, n_cr_updates=None, t_abs=-1):
        keep = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None
                for a in (p_cr, delta_m, n_cr_updates)]
        self._ck(self.lib.bpm_set_adapt_state(self._h, *[None if a is None else _dptr(a) for a in keep], int(t_abs)))

    def eval_loglike(self, X):
        X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
        assert X.shape[1] == self.dim
        out = np.empty(X.shape[0], dtype=np.float64)
        self._ck(self.lib.bpm_eval_loglike(self._h, _dptr(X), X.shape[0], _dptr(out)))
        return out

    # ---- parity hooks (test variant of the library only: HipEngine(lib=_lib.load_test())) ----------------
    def set_trace(self, on=True):
        self._need_hooks("bpm_set_trace")
        self._ck(self.lib.bpm_set_trace(self._h, 1 if on else 0))

    def get_trace(self):
        ti = np.empty((self.n_local, L.TRACE_I32), dtype=np.int32)
        tf = np.empty((self.n_local, L.TRACE_F64), dtype=np.float64)
        tm = np.empty((self.n_local, self.dim), dtype=np.uint8)
        self._ck(self.lib.bpm_get_trace(self._h, _iptr(ti), _dptr(tf), tm.ctypes.data_as(C.POINTER(C.c_uint8))))
        return dict(cr_idx=ti[:, 0], d_prime=ti[:, 1], jump=ti[:, 2], accepted=ti[:, 3], snooker=ti[:, 4],
                    partners=ti[:, 5:5 + L.MAX_PARTNERS], alpha=tf[:, 0], ll_prop=tf[:, 1], delta=tf[:, 2],
                    gamma=tf[:, 3], mask=tm.astype(bool))

    def debug_perm(self, t, shuffle=True, flip_prob=0.5):
        order = np.empty(self.n_chains, dtype=np.int32)
        inv = np.empty(self.n_chains, dtype=np.int32)
        flip = C.c_int32(0)
        self._ck(self.lib.bpm_debug_perm(self._h, int(t), 1 if shuffle else 0, float(flip_prob), _iptr(order),
                                        _iptr(inv), C.byref(flip)))
        return order, inv, bool(flip.value)

    def flavour_counts(self):
        """-> {flavour: update-kernel launches of this handle so far}, flavours that never ran left out (bpm_debug_flavour_counts; kernels.h: Flavour)"""
        self._need_hooks("bpm_debug_flavour_counts")
        out = (C.c_int64 * 7)()
        self._ck(self.lib.bpm_debug_flavour_counts(self._h, out))
        return {f: int(n) for f, n in enumerate(out) if n}


def selftest_philox(n=4096, seed=42, device=0):
    """the inline Philox against rocRAND's device engine (a test hook: runs on the test variant of the library)"""
    lib = L.load_test()
    mine = np.empty((n, 4), dtype=np.uint32)
    ref = np.empty((n, 4), dtype=np.uint32)
    L.check(lib.bpm_selftest_philox(int(device), int(n), int(seed), mine.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    ref.ctypes.data_as(C.POINTER(C.c_uint32))), lib)
    return mine, ref
