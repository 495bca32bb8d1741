"""Which flavour of the update kernel (kernels.h: Flavour, phase_fused_kernel<..., HOT>) every launch of a run takes: prepare_generation chooses it once
per generation and launch, bpm_debug_flavour_counts (test variant) counts the launches of a handle by flavour.  One case per way a configuration reaches a
flavour -- or is kept from one -- at N = 64: begin_run() with defaults, ONE step(G) call (so that the first launch of a generation folds the previous
generation's CR sums: the deferred fold, not only the dispatched one), and the counts the call added must be exactly the expected ones.  The expected
counts were recorded from the commit before the choice moved into prepare_generation, with nothing but the counter added to it.

The DREAM cases also hold p_cr, delta_m and n_cr_updates against the CPU oracle (dream.py:119-140) with the tolerances of
tests/test_gpu_shipped_path.py: a wrong plan for the CR reduction cannot hide behind right counts.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import sampler_ref as R

pytestmark = pytest.mark.gpu

N, G = 64, 12
DREAM_KW = dict(del_pairs=3, n_cr=3, burnin_gen=4, n_cr_gen=2)

# the Gaussian of independent coordinates as HIP source (tests/test_gpu_api.py: test_hip_source_likelihood_on_every_launch_path) ...
GAUSS_SRC = """__device__ double ln_like(const double* x, int d, const double* p) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) { const double z = (x[j] - p[j]) * p[d + j]; s += z * z; }
    return -0.5 * s;
}"""


def _gauss_src_ll(p, d):
    """... and in NumPy, same operations in the same order (the run-time program is compiled with unfused f64 arithmetic)"""
    def ll(x):
        s = 0.0
        for j in range(d):
            z = (x[j] - p[j]) * p[d + j]
            s += z * z
        return -0.5 * s
    return ll


def _target(name, d):
    if name == "banana":
        return R.TARGET_BANANA_2D, R.banana_params(), np.random.RandomState(1).normal(size=(N, 2)) + np.array([0.0, 1.0])
    sig = np.sqrt(np.arange(d) + 1.0)
    return R.TARGET_GAUSS_EQUICORR, R.gauss_equicorr_params(0.5, sig), np.random.RandomState(d).normal(size=(N, d)) * sig


def _added(before, after):
    return {f: after.get(f, 0) - before.get(f, 0) for f in set(before) | set(after) if after.get(f, 0) != before.get(f, 0)}


def _check_cr(eng, ora):
    st = eng.stats()
    np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)
    np.testing.assert_allclose(st["delta_m"], ora.cr.delta_m, rtol=1e-6)
    assert np.array_equal(st["n_cr_updates"], ora.cr.n_cr_updates)


# (algorithm, target, d, engine options, trace, expected counts)
SINGLE = {
    "dream_gauss100_records": (R.ALGO_DREAM, "gauss", 100, DREAM_KW, False, {3: 8, 1: 16}),
    "dream_gauss8_four_lanes_per_chain": (R.ALGO_DREAM, "gauss", 8, DREAM_KW, False, {4: 8, 2: 16}),
    "dream_gauss200_adapt_flavour_level1_from_slots": (R.ALGO_DREAM, "gauss", 200, DREAM_KW, False, {4: 8, 2: 16}),
    "dream_gauss100_four_cr_values": (R.ALGO_DREAM, "gauss", 100, dict(DREAM_KW, n_cr=4), False, {0: 24}),
    "dream_gauss600_looped_wide_kernel": (R.ALGO_DREAM, "gauss", 600, DREAM_KW, False, {0: 24}),
    "demc_gauss100": (R.ALGO_DEMC, "gauss", 100, {}, False, {1: 24}),
    "demc_banana": (R.ALGO_DEMC, "banana", 2, {}, False, {2: 24}),
    "demc_gauss100_traced": (R.ALGO_DEMC, "gauss", 100, {}, True, {0: 24}),
    "demc_sync_gauss100": (R.ALGO_DEMC_SYNC, "gauss", 100, {}, False, {0: 12}),
}


@pytest.mark.parametrize("case", sorted(SINGLE))
def test_flavours_of_a_single_gpu_run(case):
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    algo, tgt, d, kw, trace, want = SINGLE[case]
    tid, params, X0 = _target(tgt, d)
    eng = HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=params, seed=42, lib=L.load_test(), **kw)
    eng.set_state(X0)
    if trace:
        eng.set_trace(True)
    eng.begin_run()
    before = eng.flavour_counts()
    eng.step(G)
    eng.synchronize()
    got = _added(before, eng.flavour_counts())
    print(case, got)
    assert got == want
    if algo == R.ALGO_DREAM:
        ora = R.OracleSampler(algo, N, d, tid, params, 42, **kw)
        ora.set_state(X0)
        ora.run(G)
        _check_cr(eng, ora)
    eng.close()


@pytest.mark.parametrize("d,want", [(100, {5: 24}), (8, {0: 24})])
def test_flavours_of_a_rank_of_a_world(d, want):
    """Two ranks of a local group with the replay exchange (accept bytes): owner-sorted records make a rank's work items its own updates at d = 100
    (one wavefront per chain); at d = 8 the work item is the local chain and the general kernel runs."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    tid, params, X0 = _target("gauss", d)
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=R.ALGO_DEMC, n_chains=N, dim=d, target_id=tid, target_params=params, seed=42, rank=r, world_size=2, nccl_uid=uid,
                       lib=L.load_test()) for r in range(2)]
    for e in ranks:
        e.set_state(X0)
        e.begin_run()
        e.set_exchange(mode="replay")
    before = ranks[0].flavour_counts()
    arr = (C.c_void_p * 2)(*[e._h for e in ranks])
    L.check(ranks[0].lib.bpm_local_group_step(arr, 2, G), ranks[0].lib)
    ranks[0].synchronize()
    got = _added(before, ranks[0].flavour_counts())
    print("rank 0 of 2, d = %d" % d, got)
    assert got == want
    for e in ranks:
        e.close()


def test_flavours_around_a_hip_source_likelihood():
    """DREAM d = 100 with the update kernel compiled at run time around the caller's likelihood.  A module takes its burn-in flavour only in the generations
    whose CR sums the kernels write themselves -- generations 3 and 4: the gate of dream.py:123 opens n_cr_gen = 2 rows behind the start row -- and its
    general instantiation in the adapting generations before that (a shipped target has the burn-in flavour in all four: the d = 100 case above); its
    steady-state flavour with update records afterwards."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    d = 100
    p = np.concatenate([np.linspace(-1, 1, d), 1.0 / (1.0 + np.arange(d) % 3)])
    X0 = np.random.RandomState(d).normal(size=(N, d))
    eng = HipEngine(algo=R.ALGO_DREAM, n_chains=N, dim=d, target_id=R.TARGET_HOST, target_params=None, seed=42, lib=L.load_test(), **DREAM_KW)
    eng.set_state(X0)
    eng.set_device_likelihood(GAUSS_SRC, p)
    fused, why = eng.device_likelihood_info()
    assert fused, why
    eng.begin_run()
    before = eng.flavour_counts()
    eng.step(G)
    eng.synchronize()
    got = _added(before, eng.flavour_counts())
    print("hip-source likelihood", got)
    assert got == {0: 4, 3: 4, 1: 16}
    ora = R.OracleSampler(R.ALGO_DREAM, N, d, R.TARGET_HOST, None, 42, ll_fn=_gauss_src_ll(p, d), **DREAM_KW)
    ora.set_state(X0)
    ora.run(G)
    _check_cr(eng, ora)
    eng.close()

