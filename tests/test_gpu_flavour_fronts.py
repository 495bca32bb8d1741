"""The planned flavours of the one-wavefront-per-chain update kernel (kernels.h: phase_fused_kernel<ALGO, 1, 64, 2, NP, HOT>, HOT 1 / 3 / 5) that neither
tests/test_gpu_update_bits.py nor tests/test_gpu_flavours.py launches, each against the CPU oracle as tests/test_gpu_flavours.py runs its cases: DREAM with
a run-time pair count (NP = 0: del_pairs != 3) in its burn-in and steady-state flavours, and DREAM as a rank of a world (NP = 3 and NP = 0).  Their fronts
read the hot block of the argument block through whole-vector loads of their own runs (PhaseArgs; tests/test_update_kernel_arg_lines.py holds the loads to
the block's lines on the CPU): a field taken from the wrong word shows here.  64 chains, 6 generations, d = 100 and d = 65 (odd width: a pad column).

Tolerances are smoke()'s: integer decisions exact, the state to rtol 1e-10 / atol 1e-13 (the device's proposals equal the oracle's bit for bit, its ln-likes
to the order of a wavefront's sum), p_cr to rtol 1e-9."""
import ctypes as C

import numpy as np
import pytest

from oracle import sampler_ref as R

pytestmark = pytest.mark.gpu

N, G = 64, 6


def _target(d):
    sig = np.sqrt(np.arange(d) + 1.0)
    return R.TARGET_GAUSS_EQUICORR, R.gauss_equicorr_params(0.5, sig), np.random.RandomState(d).normal(size=(N, d)) * sig


def _added(before, after):
    return {f: after.get(f, 0) - before.get(f, 0) for f in set(before) | set(after) if after.get(f, 0) != before.get(f, 0)}


@pytest.mark.parametrize("d", [100, 65])
def test_dream_with_a_run_time_pair_count_on_one_gpu(d):
    """del_pairs = 2: four burn-in generations (flavour 3, two launches each), then two steady ones (flavour 1)"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    kw = dict(del_pairs=2, n_cr=3, burnin_gen=4, n_cr_gen=2)
    tid, params, X0 = _target(d)
    eng = HipEngine(algo=R.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=params, seed=42, lib=L.load_test(), **kw)
    ora = R.OracleSampler(R.ALGO_DREAM, N, d, tid, params, 42, **kw)
    eng.set_state(X0)
    ora.set_state(X0)
    eng.begin_run()
    before = eng.flavour_counts()
    eng.step(G)
    eng.synchronize()
    got = _added(before, eng.flavour_counts())
    print("del_pairs = 2, d = %d" % d, got)
    assert got == {3: 8, 1: 4}
    ora.run(G)
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted, (st["local_n_accepted"], ora.local_n_accepted)
    np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)
    eng.close()


@pytest.mark.parametrize("del_pairs", [3, 2])
@pytest.mark.parametrize("d", [100, 65])
def test_dream_as_a_rank_of_a_world(d, del_pairs):
    """Two ranks of a local group in the steady state with the replay exchange: every update launch of a rank is flavour 5, and every rank's replica of
    the state is the oracle's"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    kw = dict(del_pairs=del_pairs, n_cr=3, burnin_gen=0)
    tid, params, X0 = _target(d)
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=R.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=params, seed=42, rank=r, world_size=2, nccl_uid=uid,
                       lib=L.load_test(), **kw) for r in range(2)]
    ora = R.OracleSampler(R.ALGO_DREAM, N, d, tid, params, 42, **kw)
    ora.set_state(X0)
    for e in ranks:
        e.set_state(X0)
        e.begin_run()
        e.set_exchange(mode="replay")
    before = ranks[0].flavour_counts()
    arr = (C.c_void_p * 2)(*[e._h for e in ranks])
    L.check(ranks[0].lib.bpm_local_group_step(arr, 2, G), ranks[0].lib)
    for e in ranks:
        e.synchronize()
    got = _added(before, ranks[0].flavour_counts())
    print("rank 0 of 2, del_pairs = %d, d = %d" % (del_pairs, d), got)
    assert got == {5: 2 * G}
    ora.run(G)
    assert sum(e.stats()["local_n_accepted"] for e in ranks) == ora.local_n_accepted
    for e in ranks:
        np.testing.assert_allclose(e.get_state(), ora.X, rtol=1e-10, atol=1e-13)
    for e in ranks:
        e.close()
