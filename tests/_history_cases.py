"""What tests/test_gpu_{diagnostics,quantiles,covariance,histograms}.py share: the engine and the sampler whose history a statistic is taken
over, the statistics' host class over a bare engine (_over), the local group of ranks over the push exchange with its single-rank twin, and the launcher of rank processes (tests/_stats_worker.py).
A plain module: the tests import what they use."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

GROUP_CASE = "dream_gauss100_long"      # (tests/_push_worker.py: case_spec)
CHILD_LIMIT_S = 300                     # one child process; the Python-side limit sits above `timeout`'s own


def _engine(N, d, G=None, **kw):
    """a DREAM engine on the equicorrelated Gaussian; G (the generations the caller is about to install or step) is not needed to build it"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, _ = d100_gauss.Gauss_100D(rho=0.5, dim=d)._bpm_target_spec()
    return HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=5, **kw)


def _over(engine):
    """the statistics' host class over a bare engine of one rank"""
    from bipymc_amd._history_stats import HistoryStatistics
    from bipymc_amd.comm import single_process_allgather

    class Over(HistoryStatistics):
        n_chains = engine.n_chains
        _stats_allgather = staticmethod(single_process_allgather)

        def _stats_engine(self, who):
            return engine

    return Over()


def _dream_class(N, d, gens, shuffle=True, rho=0.5, n_burn=0):
    """DreamMpi after `gens` generations (n_burn: the caller's own, not used to run)"""
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=rho, dim=d)
    s = DreamMpi(t.ln_like, np.zeros(d), n_chains=N, n_cr_gen=10, burnin_gen=50, seed=21)
    s.run_mcmc(N * (gens + 1), shuffle=shuffle)
    return s


def local_group(R):
    """R ranks as handles of this process over the push exchange (the test variant's local group), stepped as tests/_push_worker.py does
    -> (ranks, N, d); the caller closes them"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from _push_worker import case_spec, start_state
    spec, algo, N, kw, G = case_spec(GROUP_CASE)
    tid, tp, d = spec
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, rank=r, world_size=R, nccl_uid=uid,
                       lib=L.load_test(), **kw) for r in range(R)]
    blobs = [e.push_export() for e in ranks]
    for e in ranks:
        e.push_connect(blobs)
    arr = (C.c_void_p * R)(*[e._h for e in ranks])
    ok = C.c_int32(0)
    L.check(ranks[0].lib.bpm_push_selftest(arr, R, C.byref(ok)), ranks[0].lib)
    assert ok.value == 1
    x0 = start_state(GROUP_CASE, N, d)
    for e in ranks:
        e.set_state(x0)
        e.begin_run(flip=0.4)
    L.check(ranks[0].lib.bpm_local_group_step(arr, R, G), ranks[0].lib)
    return ranks, N, d


def per_rank(ranks, method):
    """-> f(*args) = [rank.method(*args) for every rank]: a statistic's per-rank call as a communicator's allgather hands its parts out"""
    return lambda *args: [getattr(e, method)(*args) for e in ranks]


def group_single_rank():
    """the one-rank engine that ran what local_group's ranks ran together; the caller closes it"""
    from bipymc_amd.engine import HipEngine
    from _push_worker import case_spec, start_state
    spec, algo, N, kw, G = case_spec(GROUP_CASE)
    tid, tp, d = spec
    one = HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, **kw)
    one.set_state(start_state(GROUP_CASE, N, d))
    one.begin_run(flip=0.4)
    one.step(G)
    return one


def run_rank_processes(tmp_path, stat):
    """tests/_stats_worker.py <stat>: one single-rank process, then two ranks together, every child under `timeout -k 10`; nothing more is
    started after a child that did not exit with 0.  -> (the one-rank world's .npz, [the two ranks' .npz])"""
    from _stats_worker import STATS
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["BPM_PUSH_TIMEOUT_S"] = "60"
    d_ = str(tmp_path)

    def child(rank, world):
        return ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(HERE, "_stats_worker.py"), stat, d_, str(rank), str(world)]

    subprocess.check_call(child(0, 1), env=env, timeout=CHILD_LIMIT_S + 30)
    procs = [subprocess.Popen(child(r, 2), env=env) for r in range(2)]
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=CHILD_LIMIT_S + 30))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert codes == [0, 0], codes
    name = os.path.join(d_, STATS[stat][1] + "_w%d_rank%d.npz")
    return np.load(name % (1, 0)), [np.load(name % (2, k)) for k in range(2)]
