"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the
same seeds.  Bit-exact on every integer quantity; float tolerances are written at each assert.

Run on the GPU box with `pytest -m gpu`."""
import json
import os

import numpy as np
import pytest

from oracle import philox_ref as P
from oracle import sampler_ref as R

pytestmark = pytest.mark.gpu

RTOL_STEP = 1e-12      # one generation: only libm (log/cos/exp) and reduction-order differences
ATOL_STEP = 1e-15


def _engine(**kw):
    from bipymc_amd.engine import HipEngine
    return HipEngine(**kw)


def _hooks_engine(**kw):
    """an engine on the TEST VARIANT of the library (build_variants/libbipymc_test.so, include/bipymc_hip_test.h): the product library
    exports no bpm_debug_* entry point"""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    return HipEngine(lib=L.load_test(), **kw)


def _gauss_params(d, rho=0.5):
    return R.gauss_equicorr_params(rho, np.sqrt(np.arange(d) + 1.0))


def _mix_params():
    return R.mixture_pairs_params(0.25, 0.75, [0, 0], [2, 2], [0.25, 0.25], [0.25, 0.25], 0.8, -0.8)


def _pair(algo, N, d, target_id, params, seed, hooks=False, **kw):
    """(HipEngine, OracleSampler) with identical configuration.  hooks=True: the engine runs on the test variant of the library (the per-chain
    decision trace, bpm_set_trace / bpm_get_trace, is part of the test surface: include/bipymc_hip_test.h)."""
    eng = (_hooks_engine if hooks else _engine)(algo=algo, n_chains=N, dim=d, target_id=target_id, target_params=params, seed=seed, **kw)
    okw = {k: v for k, v in kw.items() if k in ("gamma_scale", "del_pairs", "burnin_gen", "n_cr_gen", "n_cr", "p_snooker", "outlier_every")}
    ora = R.OracleSampler(algo, N, d, target_id, params, seed, **okw)
    return eng, ora


def _pair_traced(*a, **kw):
    return _pair(*a, hooks=True, **kw)


# ------------------------------------------------------------------ RNG layer
def test_philox_equals_rocrand_on_device():
    from bipymc_amd.engine import selftest_philox
    mine, ref = selftest_philox(n=8192, seed=0x1234567890ABCDEF)
    assert np.array_equal(mine, ref)                      # inline Philox == rocRAND device engine, bit for bit
    # and both equal the oracle's statement of the same blocks
    i = np.arange(8192, dtype=np.uint64)
    subseq = np.where(i % 3 == 0, P.SUBSEQ_GLOBAL, i * np.uint64(2654435761))
    blk = ((i * np.uint64(37)) << np.uint64(16)) | (i % np.uint64(120))
    exp = P.block(0x1234567890ABCDEF, subseq, blk)
    assert np.array_equal(mine, exp)


@pytest.mark.parametrize("N", [4, 5, 10, 64, 1000, 8192, 65536])
def test_shuffle_and_flip_bit_exact(N):
    eng = _hooks_engine(algo=R.ALGO_DEMC, n_chains=N, dim=2, target_id=R.TARGET_BANANA_2D, target_params=R.banana_params(), seed=99)
    for t in (0, 1, 17, 70000):
        order, inv, flip = eng.debug_perm(t, True, 0.5)
        exp = P.shuffle_idx(99, t, N)
        assert np.array_equal(order, exp)
        assert np.array_equal(inv, P.perm_inv(np.arange(N), N, P.shuffle_keys(99, t)))
        assert flip == P.flip_draw(99, t, 0.5)
    order, inv, _ = eng.debug_perm(3, False, 0.5)
    assert np.array_equal(order, np.arange(N)) and np.array_equal(inv, np.arange(N))


# ------------------------------------------------------------------ targets
def test_targets_against_reference_known_answers(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "targets_known_answers.json")))
    eng = _engine(algo=R.ALGO_DREAM, n_chains=8, dim=100, target_id=R.TARGET_GAUSS_EQUICORR, target_params=_gauss_params(100), seed=1)
    X = np.array([e["x"] for e in g["Gauss_100D"]])
    ll = eng.eval_loglike(X)
    # tolerance 1e-12 relative: O(d) closed form vs the reference's scipy evaluation
    np.testing.assert_allclose(ll, [e["logpdf_true"] for e in g["Gauss_100D"]], rtol=1e-12)
    eng = _engine(algo=R.ALGO_DREAM, n_chains=8, dim=16, target_id=R.TARGET_GAUSS_EQUICORR, target_params=_gauss_params(16), seed=1)
    np.testing.assert_allclose(eng.eval_loglike(np.array([e["x"] for e in g["Gauss_16D"]])),
                               [e["ln_like"] for e in g["Gauss_16D"]], rtol=1e-12)
    eng = _engine(algo=R.ALGO_DREAM, n_chains=8, dim=2, target_id=R.TARGET_MIXTURE_PAIRS, target_params=_mix_params(), seed=1)
    np.testing.assert_allclose(eng.eval_loglike(np.array([e["x"] for e in g["BimodeGauss_2D"]])),
                               [e["ln_like"] for e in g["BimodeGauss_2D"]], rtol=1e-12)
    eng = _engine(algo=R.ALGO_DEMC, n_chains=8, dim=2, target_id=R.TARGET_BANANA_2D, target_params=R.banana_params(sigma1=1.0, sigma2=1.0), seed=1)
    np.testing.assert_allclose(eng.eval_loglike(np.array([e["x"] for e in g["Banana_2D"]])),
                               [e["ln_like"] for e in g["Banana_2D"]], rtol=1e-12)


@pytest.mark.parametrize("d", [1, 2, 3, 7, 8, 16, 33, 100, 128, 130, 256, 300, 512, 513, 1000, 1024, 1025, 1999, 2048])
def test_gauss_target_every_kernel_shape(d):
    """every (lanes-per-chain, dims-per-lane) instantiation, odd dims (padded rows) included"""
    params = _gauss_params(d, rho=0.3)
    eng = _engine(algo=R.ALGO_DREAM, n_chains=8, dim=d, target_id=R.TARGET_GAUSS_EQUICORR, target_params=params, seed=1)
    X = np.random.RandomState(d).normal(size=(37, d)) * np.sqrt(np.arange(d) + 1.0)
    np.testing.assert_allclose(eng.eval_loglike(X), R.ll_gauss_equicorr(X, params), rtol=1e-13)


@pytest.mark.parametrize("d", [2, 4, 8, 32, 100, 600, 1026, 2048])
def test_mixture_target_shapes(d):
    eng = _engine(algo=R.ALGO_DREAM, n_chains=8, dim=d, target_id=R.TARGET_MIXTURE_PAIRS, target_params=_mix_params(), seed=1)
    rs = np.random.RandomState(d)
    X = np.where(rs.uniform(size=(50, 1)) < 0.5, 0.0, 2.0) + 0.3 * rs.normal(size=(50, d))
    np.testing.assert_allclose(eng.eval_loglike(X), R.ll_mixture_pairs(X, _mix_params()), rtol=1e-12)


# ------------------------------------------------------------------ init
@pytest.mark.parametrize("d,N", [(2, 10), (100, 64), (7, 12)])
def test_init_jitter(d, N):
    eng, ora = _pair(R.ALGO_DREAM, N, d, R.TARGET_GAUSS_EQUICORR, _gauss_params(d), 5)
    theta0 = np.linspace(-1, 1, d)
    var = np.full(d, 1e-6) * (1 + np.arange(d))
    eng.init_chains(theta0, var)
    ora.init_jitter(theta0, var)
    # 1e-13 relative: Box-Muller log/cos of two libms
    np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-13, atol=0)
    np.testing.assert_allclose(eng.get_loglike(), ora.ll, rtol=1e-12)
    eng.init_chains(theta0, np.zeros(d))      # util.py:12: no noise unless all variances > 0
    assert np.array_equal(eng.get_state(), np.tile(theta0, (N, 1)))


# ------------------------------------------------------------------ one generation, everything
def _collect_oracle_trace(tr, N, d, n_part):
    out = dict(cr_idx=np.full(N, -1), d_prime=np.full(N, d), jump=np.zeros(N, int), accepted=np.zeros(N, int),
               snooker=np.zeros(N, int), partners=np.full((N, n_part), -1), mask=np.zeros((N, d), bool),
               alpha=np.zeros(N), ll_prop=np.zeros(N), delta=np.zeros(N))
    for ph in ("phase0", "phase1"):
        r = tr[ph]
        ids = r["ids"]
        out["jump"][ids] = r["jump"]
        out["accepted"][ids] = r["accepted"]
        out["alpha"][ids] = r["alpha"]
        out["ll_prop"][ids] = r["ll_prop"]
        out["delta"][ids] = r["delta"]
        if "cr_idx" in r:
            out["cr_idx"][ids] = r["cr_idx"]
            out["d_prime"][ids] = r["d_prime"]
            out["mask"][ids] = r["mask"]
            P_ = r["pa"].shape[1]
            out["partners"][ids[:, None], 2 * np.arange(P_)[None, :]] = r["pa"]
            out["partners"][ids[:, None], 2 * np.arange(P_)[None, :] + 1] = r["pb"]
        else:
            out["partners"][ids, 0] = r["pa"]
            out["partners"][ids, 1] = r["pb"]
            if "snooker" in r:
                out["snooker"][ids] = r["snooker"]
                out["partners"][ids, 2] = r["iz"]
                out["partners"][ids, 3] = r["i1"]
                out["partners"][ids, 4] = r["i2"]
    return out


def _check_generation(eng, ora, N, d, dream, n_part):
    # the per-generation normal jitter is evaluated in float32 (hardware log2/sin/cos on the device,
    # NumPy float32 in the oracle): they agree to ~1e-6 relative, i.e. 1e-5 * epsilon absolute
    atol_state = max(ATOL_STEP, 1e-5 * ora._run_args[2])
    ora.trace = []
    eng.step(1)
    ora._generation(ora._k, *ora._run_args)
    ora._k += 1
    tr = eng.get_trace()
    exp = _collect_oracle_trace(ora.trace[-1], N, d, n_part)
    # ---- integer decisions: bit-exact
    assert np.array_equal(tr["partners"][:, :n_part], exp["partners"])
    assert np.array_equal(tr["jump"], exp["jump"])
    if dream:
        assert np.array_equal(tr["cr_idx"], exp["cr_idx"])
        assert np.array_equal(tr["d_prime"], exp["d_prime"])
        assert np.array_equal(tr["mask"], exp["mask"])
    else:
        assert np.array_equal(tr["snooker"], exp["snooker"])
    assert np.array_equal(tr["accepted"], exp["accepted"])
    # ---- floats: 1e-12 relative (libm + reduction order only)
    np.testing.assert_allclose(tr["ll_prop"], exp["ll_prop"], rtol=RTOL_STEP, atol=max(1e-12, 1e3 * atol_state))
    np.testing.assert_allclose(tr["alpha"], exp["alpha"], rtol=1e-8, atol=1e-300)   # exp() of an O(100) difference
    # delta divides by the chain's own history variance: for a chain that has barely moved this is ~1e-30 and
    # amplifies the (1e-19 absolute) float32-jitter difference between device and oracle
    np.testing.assert_allclose(tr["delta"], exp["delta"], rtol=1e-6)
    X1 = eng.get_state()
    np.testing.assert_allclose(X1, ora.X, rtol=RTOL_STEP, atol=atol_state)
    np.testing.assert_allclose(eng.get_loglike(), ora.ll, rtol=RTOL_STEP, atol=max(1e-12, 1e3 * atol_state))
    return float(np.mean(X1 == ora.X))


def _start(eng, ora, X, **run):
    eng.set_state(X)
    ora.set_state(X)
    eng.set_trace(True)
    eng.begin_run(**run)
    ora.local_n_accepted, ora.local_n_rejected = 0, 1
    ora._k = 0
    eps = run.get("epsilon", None)
    if eps is None:
        eps = 1e-12 if ora.algo == R.ALGO_DREAM else 1e-15
    ora._run_args = (float(np.clip(run.get("flip", 0.5), 0, 1)), run.get("shuffle", True), float(eps),
                     float(run.get("u_epsilon", 1e-2) if run.get("u_epsilon", None) is not None else 1e-2),
                     run.get("gamma", None))


@pytest.mark.parametrize("d,N,P_", [(100, 64, 3), (100, 10, 3), (2, 10, 3), (8, 32, 3), (16, 24, 1), (6, 9, 5),
                                    (130, 16, 2), (5, 20, 3), (300, 8, 3)])
def test_dream_generation_parity(d, N, P_):
    eng, ora = _pair_traced(R.ALGO_DREAM, N, d, R.TARGET_GAUSS_EQUICORR, _gauss_params(d), 1234, del_pairs=P_,
                     burnin_gen=100, n_cr_gen=3, n_cr=3)
    X = np.random.RandomState(0).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0)
    _start(eng, ora, X)
    exact = []
    for g in range(12):       # k = 0, 5, 10 take the gamma=1 branch; CR statistic switches on at history length 4
        exact.append(_check_generation(eng, ora, N, d, True, 2 * P_))
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected
    np.testing.assert_allclose(st["n_cr_updates"], ora.cr.n_cr_updates, rtol=0)
    np.testing.assert_allclose(st["delta_m"], ora.cr.delta_m, rtol=1e-9)
    np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)
    assert ora.cr.n_cr_updates.sum() > 0
    print("fraction of state entries bit-identical to the oracle per generation:", exact)


@pytest.mark.parametrize("N", [20000, 70000])
def test_cr_adaptation_two_stage_reduction_matches_oracle(N):
    """The per-generation CR reduction in both of its forms -- up to 65536 chains partial sums by up to 64 workgroups + one folding
    wavefront in a second dispatch (N = 20000: 40 workgroups of 512 chains), beyond that ONE dispatch whose last workgroup to finish
    folds (N = 70000: 35 workgroups of 2048 chains) -- gives the same decisions, delta_m and p_cr as the oracle."""
    d = 2
    eng, ora = _pair_traced(R.ALGO_DREAM, N, d, R.TARGET_GAUSS_EQUICORR, _gauss_params(d), 77, del_pairs=3, burnin_gen=100, n_cr_gen=2, n_cr=3)
    X = np.random.RandomState(5).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0)
    _start(eng, ora, X)
    for g in range(6):
        _check_generation(eng, ora, N, d, True, 6)
    st = eng.stats()
    assert ora.cr.n_cr_updates.sum() > 3 * N
    np.testing.assert_allclose(st["n_cr_updates"], ora.cr.n_cr_updates, rtol=0)
    np.testing.assert_allclose(st["delta_m"], ora.cr.delta_m, rtol=1e-9)
    np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)


def test_dream_mixture_generation_parity():
    N, d = 40, 8
    eng, ora = _pair_traced(R.ALGO_DREAM, N, d, R.TARGET_MIXTURE_PAIRS, _mix_params(), 77, burnin_gen=4, n_cr_gen=2)
    rs = np.random.RandomState(3)
    X = np.where(rs.uniform(size=(N, 1)) < 0.5, 0.0, 2.0) + 0.3 * rs.normal(size=(N, d))
    _start(eng, ora, X)
    for g in range(8):          # adaptation stops after generation 4 (burnin_gen)
        _check_generation(eng, ora, N, d, True, 6)
    np.testing.assert_allclose(eng.stats()["p_cr"], ora.cr.p_cr, rtol=1e-9)


@pytest.mark.parametrize("N,p_snk", [(8, 0.0), (64, 0.0), (64, 0.3), (1001, 0.1)])
def test_demc_banana_generation_parity(N, p_snk):
    eng, ora = _pair_traced(R.ALGO_DEMC, N, 2, R.TARGET_BANANA_2D, R.banana_params(), 4321, p_snooker=p_snk)
    rs = np.random.RandomState(5)
    X = rs.normal(size=(N, 2)) * np.array([1.1, 1.1]) + np.array([0.0, 1.2])
    _start(eng, ora, X)
    for g in range(11):         # k = 0 and 10 take the gamma = 1 branch
        _check_generation(eng, ora, N, 2, False, 5 if p_snk > 0 else 2)
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted


@pytest.mark.parametrize("N,P_,n_cr", [(10, 3, 3), (40, 3, 3), (33, 2, 4), (64, 1, 1)])
def test_dream_banana_generation_parity(N, P_, n_cr):
    """DREAM on the banana -- the reference's own scenario tests/test_banana.py:123-127 (DreamMpi, n_chains = 10) -- had no GPU test (VERDICT r04
    weak 1): kernels launch_fused<ALGO_DREAM, TARGET_BANANA, 3 | 0, 1, 2> (sampler.hip: g_fused_banana[1], [2]), one lane per chain, always in the lean form
    (ln-like re-evaluated from the own row).  Every decision of every update over 12 generations, CR adaptation switching on at history length 3 and
    off after generation 8 (dream.py:92,123)."""
    eng, ora = _pair_traced(R.ALGO_DREAM, N, 2, R.TARGET_BANANA_2D, R.banana_params(), 2468, del_pairs=P_, burnin_gen=8, n_cr_gen=2, n_cr=n_cr)
    rs = np.random.RandomState(6)
    X = rs.normal(size=(N, 2)) * np.array([1.1, 1.1]) + np.array([0.0, 1.2])
    _start(eng, ora, X)
    for g in range(12):
        _check_generation(eng, ora, N, 2, True, 2 * P_)
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected
    np.testing.assert_allclose(st["n_cr_updates"], ora.cr.n_cr_updates, rtol=0)
    np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)
    assert n_cr == 1 or ora.cr.n_cr_updates.sum() > 0


@pytest.mark.parametrize("N,d,p_snk", [(20, 2, 0.0), (20, 2, 0.3), (48, 8, 0.1), (30, 30, 0.2), (24, 130, 0.0), (16, 514, 0.25)])
def test_demc_mixture_generation_parity(N, d, p_snk):
    """DE-MC on the bimodal mixture -- tests/test_dblgauss.py:130-133 (DeMcMpi, n_chains = 20) -- ran only in a statistical scenario:
    g_fused_mixture[0][*], d = 2 (the reference's BimodeGauss_2D), 8, 30, 130 and the looped wide-row kernel at d = 514.  Every decision of every update
    over 11 generations (k = 0 and 10 take the gamma = 1 branch, demc.py:174-177), with and without snooker updates."""
    eng, ora = _pair_traced(R.ALGO_DEMC, N, d, R.TARGET_MIXTURE_PAIRS, _mix_params(), 1357, p_snooker=p_snk)
    rs = np.random.RandomState(7)
    X = np.where(rs.uniform(size=(N, 1)) < 0.3, 0.0, 2.0) + 0.3 * rs.normal(size=(N, d))
    _start(eng, ora, X)
    for g in range(11):
        _check_generation(eng, ora, N, d, False, 5 if p_snk > 0 else 2)
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected


def test_demc_gauss_with_options():
    """run_mcmc kwargs: flip, shuffle, epsilon, gamma (demc.py:73-75,161-162)"""
    N, d = 30, 16
    eng, ora = _pair_traced(R.ALGO_DEMC, N, d, R.TARGET_GAUSS_EQUICORR, _gauss_params(d), 8)
    X = np.random.RandomState(1).normal(size=(N, d))
    _start(eng, ora, X, flip=1.0, shuffle=False, epsilon=1e-6, gamma=0.4)
    for g in range(3):
        _check_generation(eng, ora, N, d, False, 2)
    _start(eng, ora, X, flip=0.0, shuffle=True, epsilon=0.0)
    for g in range(3):
        _check_generation(eng, ora, N, d, False, 2)


@pytest.mark.parametrize("algo,d,N,n_chunks,kw", [
    (R.ALGO_DREAM, 10, 24, 1, dict(del_pairs=3, burnin_gen=5, n_cr_gen=2)),
    (R.ALGO_DREAM, 10, 24, 3, dict(del_pairs=3, burnin_gen=5, n_cr_gen=2)),
    (R.ALGO_DREAM, 7, 50, 7, dict(del_pairs=2, burnin_gen=100, n_cr_gen=1)),           # odd d: padded rows in the staging
    (R.ALGO_DREAM, 100, 64, 4, dict(del_pairs=3, burnin_gen=4, n_cr_gen=2)),
    (R.ALGO_DREAM, 600, 12, 5, dict(del_pairs=3, burnin_gen=4, n_cr_gen=2)),          # the looped wide-row kernels
    (R.ALGO_DEMC, 3, 33, 4, dict(p_snooker=0.3)),
    (R.ALGO_DEMC, 2, 9, 9, dict(p_snooker=0.0)),                                       # more chunks than some halves have rows: empty pieces
])
def test_chunked_read_back_of_the_host_callback_path_against_oracle(algo, d, N, n_chunks, kw):
    """Round 5: the half generation's proposals come back in pieces (bpm_propose_begin / bpm_propose_chunk: the DMA of piece
    k + 1 under the caller's evaluation of piece k), the ln-likes go in piece by piece IN ANY ORDER (bpm_commit_chunk), bpm_commit_end finishes --
    against OracleSampler(ll_fn=...) like the one-piece form above: every accept decision exact, states / history to 1e-11."""
    params = _gauss_params(d, rho=0.4)

    def py_ll(theta):
        return float(R.ll_gauss_equicorr(theta, params))

    eng = _engine(algo=algo, n_chains=N, dim=d, target_id=R.TARGET_HOST, target_params=None, seed=78, **kw)
    okw = {k: v for k, v in kw.items() if k in ("del_pairs", "burnin_gen", "n_cr_gen", "p_snooker")}
    ora = R.OracleSampler(algo, N, d, R.TARGET_HOST, None, 78, ll_fn=py_ll, **okw)
    X0 = np.random.RandomState(4).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0)
    eng.set_state(X0)
    eng.set_loglike(np.array([py_ll(x) for x in X0]))
    ora.set_state(X0)
    eng.begin_run()
    seen_rows = 0
    for g in range(9):
        for ph in range(2):
            pieces = [(k, rows.copy(), ids.copy()) for k, rows, ids in eng.propose_chunks(n_chunks)]
            assert [p[0] for p in pieces] == list(range(n_chunks)) and all(p[1].shape == (len(p[2]), d) for p in pieces)
            assert all(np.all(p[2] >= 0) for p in pieces)                 # one rank: every work item is active
            seen_rows += sum(len(p[2]) for p in pieces)
            for k, rows, ids in reversed(pieces):                        # (the values may be handed in in any order)
                eng.commit_chunk(k, np.array([py_ll(r) for r in rows]))
            eng.commit_end()
        ora._generation(g, 0.5, True, 1e-12 if algo == R.ALGO_DREAM else 1e-15, 1e-2, None)
        np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-11, atol=1e-13)
    assert seen_rows == 9 * N
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected
    if algo == R.ALGO_DREAM:
        np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-7 if d > 512 else 1e-9)
    np.testing.assert_allclose(eng.get_history(), ora.history_array(), rtol=1e-11, atol=1e-13)
    # misuse is an error, not a hang or a silent half generation
    from bipymc_amd._lib import BpmError
    it = eng.propose_chunks(2)
    k0, rows0, _ids0 = next(it)
    with pytest.raises(BpmError, match="chunks were given"):
        eng.commit_end()
    eng.commit_chunk(k0, np.zeros(len(rows0)))
    with pytest.raises(BpmError, match="handed in already"):
        eng.commit_chunk(k0, np.zeros(len(rows0)))
    with pytest.raises(BpmError, match="another entry point"):
        eng.commit(np.zeros(N))


@pytest.mark.parametrize("algo,d,N,kw", [
    (R.ALGO_DREAM, 10, 24, dict(del_pairs=3, burnin_gen=5, n_cr_gen=2)),
    (R.ALGO_DREAM, 101, 40, dict(del_pairs=3, burnin_gen=4, n_cr_gen=2)),              # odd d: a row stride of 102 doubles in device memory
    (R.ALGO_DEMC, 4, 30, dict(p_snooker=0.2)),
])
def test_device_resident_likelihood_against_oracle(algo, d, N, kw):
    """Round 5: the likelihood evaluated ON THE DEVICE by the caller's framework -- the proposals are handed over where they lie
    (engine.DeviceRows: `__cuda_array_interface__`, wrapped by torch without a copy), the ln-likes come back as a device tensor
    (bpm_propose_device / bpm_commit_device): no PCIe.  Against OracleSampler(ll_fn=...) with the same formula in NumPy: accept counts equal, state
    and history to 1e-10 (torch's and NumPy's row sums differ in the last bits).  In a child process that imports torch FIRST: the torch wheel carries
    a HIP runtime of its own, and a process can initialise only one (the library then binds to the one already loaded) -- the order a user's script has."""
    import importlib.util
    if importlib.util.find_spec("torch") is None:      # (NOT imported here: torch brings HIP / HSA / RCCL copies of its own, and importing it into a process
        pytest.skip("PyTorch is not installed")       #  whose library is already loaded breaks RCCL's first contact for every later test)
    import json as _json
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "_torch_worker.py"), "device_parity", str(algo), str(d), str(N), _json.dumps(kw)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and b"device_parity ok" in r.stdout, r.stdout.decode()[-3000:]


# ------------------------------------------------------------------ history, results
def test_history_rows_and_super_chain_order():
    N, d, G = 12, 6, 9
    eng, ora = _pair(R.ALGO_DREAM, N, d, R.TARGET_GAUSS_EQUICORR, _gauss_params(d), 3, burnin_gen=0)
    X = np.random.RandomState(2).normal(size=(N, d))
    eng.set_state(X); ora.set_state(X)
    eng.begin_run(); eng.step(G); ora.run(G)
    H = eng.get_history()
    assert H.shape == (G + 1, N, d)
    assert np.array_equal(H[0], X)                             # row 0 = initial state (chain.py:29)
    assert np.array_equal(H[-1], eng.get_state())              # last row = current_pos (chain.py:122-124)
    np.testing.assert_allclose(H, ora.history_array(), rtol=1e-10, atol=1e-14)
    llh = eng.get_loglike_history()
    np.testing.assert_allclose(llh, np.stack(ora.ll_history), rtol=1e-10, atol=1e-12)
    # second run_mcmc call continues the history, k restarts (demc.py:78): gamma jump at k = 0 again
    eng.begin_run(); eng.step(2); ora.run(2)
    assert eng.history_rows() == G + 3
    np.testing.assert_allclose(eng.get_history(), ora.history_array(), rtol=1e-9, atol=1e-13)
    st = eng.stats()
    assert st["k_gen"] == 2 and st["t_abs"] == G + 2
    assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected


def test_cr_adaptation_resumes_after_gap():
    """burn-in gating restarts with k on every run_mcmc (demc.py:78, dream.py:92): the Welford
    moments must be rebuilt from the stored history when adaptation resumes."""
    N, d = 16, 4
    eng, ora = _pair(R.ALGO_DREAM, N, d, R.TARGET_GAUSS_EQUICORR, _gauss_params(d), 21, burnin_gen=3, n_cr_gen=2)
    X = np.random.RandomState(4).normal(size=(N, d))
    eng.set_state(X); ora.set_state(X)
    for _ in range(2):
        eng.begin_run(); eng.step(7); ora.run(7)       # 3 adapting generations, 4 without, twice
        st = eng.stats()
        np.testing.assert_allclose(st["n_cr_updates"], ora.cr.n_cr_updates, rtol=0)
        np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-8)
    np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-9, atol=1e-13)


def test_no_history_mode():
    N, d = 16, 4
    eng = _engine(algo=R.ALGO_DEMC, n_chains=N, dim=d, target_id=R.TARGET_GAUSS_EQUICORR, target_params=_gauss_params(d),
                  seed=2, keep_history=False)
    ora = R.OracleSampler(R.ALGO_DEMC, N, d, R.TARGET_GAUSS_EQUICORR, _gauss_params(d), 2)
    X = np.random.RandomState(4).normal(size=(N, d))
    eng.set_state(X); ora.set_state(X)
    eng.begin_run(); eng.step(5); ora.run(5)
    assert eng.history_rows() == 1
    np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-10, atol=1e-14)


def test_errors_are_reported_not_thrown():
    from bipymc_amd._lib import BpmError
    with pytest.raises(BpmError):
        _engine(algo=R.ALGO_DEMC, n_chains=3, dim=2, target_id=R.TARGET_BANANA_2D, target_params=R.banana_params(), seed=1)
    with pytest.raises(BpmError):
        _engine(algo=R.ALGO_DEMC, n_chains=8, dim=3, target_id=R.TARGET_BANANA_2D, target_params=R.banana_params(), seed=1)
    eng = _engine(algo=R.ALGO_DEMC, n_chains=8, dim=2, target_id=R.TARGET_BANANA_2D, target_params=R.banana_params(), seed=1)
    with pytest.raises(BpmError, match="not initilized"):
        eng.begin_run()
    eng.init_chains(np.zeros(2), 1e-6)
    with pytest.raises(BpmError):
        eng.step(1)                 # begin_run first
    with pytest.raises(BpmError):
        eng.get_history(0, 5)
    # exchange policy: a single-GPU sampler only has the dense (no-op) exchange; bad modes are refused
    import ctypes as C
    xs = eng.exchange_stats()
    assert (xs["mode"], xs["cap"], xs["chunks"], xs["replays"], xs["replay_gens"], xs["push_gens"], xs["push_connected"]) == ("dense", 0, 0, 0, 0, 0, False)
    eng.set_exchange(mode="dense")
    with pytest.raises(BpmError, match="dense exchange"):
        eng.set_exchange(mode="replay")
    assert eng.lib.bpm_set_exchange(eng._h, C.c_int32(7), C.c_int32(0)) != 0
    with pytest.raises(ValueError):
        _engine(algo=R.ALGO_DEMC, n_chains=8, dim=2, target_id=R.TARGET_BANANA_2D, target_params=R.banana_params(), seed=1,
                world_size=3, rank=0, nccl_uid=b"BPMLOCAL" + bytes(120))           # n_chains % world_size != 0 (refused by the wrapper before any library call)


def test_outlier_chain_reset_matches_oracle():
    """DREAM outlier-chain reset (extension; absent from the reference): chains parked far in the tails are
    detected by the IQR rule on their mean ln_like and restart from the best chain; engine == oracle."""
    N, d = 32, 8
    eng, ora = _pair(R.ALGO_DREAM, N, d, R.TARGET_MIXTURE_PAIRS, _mix_params(), 3, burnin_gen=200, n_cr_gen=10,
                     outlier_every=20)
    rs = np.random.RandomState(0)
    X = np.where(rs.uniform(size=(N, 1)) < 0.25, 0.0, 2.0) + 0.25 * rs.normal(size=(N, d))
    X[5] = 30.0
    X[17] = -25.0
    eng.set_state(X); ora.set_state(X)
    eng.begin_run(); eng.step(100); ora.run(100)
    st = eng.stats()
    assert st["n_outlier_resets"] == ora.n_outlier_resets >= 2
    np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(eng.get_loglike(), ora.ll, rtol=1e-8, atol=1e-9)
    H = eng.get_history()
    assert np.array_equal(H[-1], eng.get_state())
    np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-7)
    assert np.all(eng.get_loglike() > -50)          # nobody is left in the tails


@pytest.mark.parametrize("N,d,P_,n_cr", [(4, 1, 1, 1), (5, 3, 1, 2), (4, 100, 1, 3), (7, 2, 3, 8), (23, 9, 10, 3),
                                         (6, 512, 2, 3), (11, 511, 3, 3), (64, 114, 3, 3), (64, 116, 3, 3), (16, 128, 3, 5),
                                         (7, 513, 3, 3), (6, 1024, 2, 3), (9, 1025, 3, 3), (5, 1500, 1, 2), (8, 2048, 3, 3)])
def test_dream_edge_shapes(N, d, P_, n_cr):
    """smallest populations (pool of two), odd N (unequal pools), dim 1, padded odd dims, the largest dims (8 and 16 coordinate pairs per lane: d up to 2048),
    del_pairs up to 10, n_cr 1..8, and the dims around the merged-Philox lane budget (114 / 116)."""
    if 2 * P_ > 0 and (N // 2) < 2:
        pytest.skip("pool too small")
    eng, ora = _pair_traced(R.ALGO_DREAM, N, d, R.TARGET_GAUSS_EQUICORR, _gauss_params(d), 99, del_pairs=P_, burnin_gen=6,
                     n_cr_gen=2, n_cr=n_cr)
    X = np.random.RandomState(1).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0)
    _start(eng, ora, X)
    for g in range(8):
        _check_generation(eng, ora, N, d, True, 2 * P_)
    np.testing.assert_allclose(eng.stats()["p_cr"], ora.cr.p_cr, rtol=1e-6)


@pytest.mark.parametrize("N,d", [(4, 1), (5, 2), (6, 3), (9, 100), (8, 300), (7, 777), (6, 2047)])
def test_demc_edge_shapes(N, d):
    eng, ora = _pair_traced(R.ALGO_DEMC, N, d, R.TARGET_GAUSS_EQUICORR, _gauss_params(d), 98, p_snooker=0.5)
    X = np.random.RandomState(2).normal(size=(N, d))
    _start(eng, ora, X)
    for g in range(11):
        _check_generation(eng, ora, N, d, False, 5)


@pytest.mark.parametrize("N,d,tgt", [(8, 2, "banana"), (64, 2, "banana"), (33, 16, "gauss"), (10, 100, "gauss"), (5, 3, "gauss"),
                                     (48, 200, "gauss"), (40, 400, "gauss"), (24, 640, "gauss"), (16, 1025, "gauss"),      # two / four pairs per lane, the looped kernel
                                     (33, 8, "mix"), (24, 130, "mix"), (16, 514, "mix")])
def test_demc_sync_mode_parity(N, d, tgt):
    """Synchronous DE-MC (serial `DeMc` of samplers.py:237-308, delayed_accept=True): pair from all OTHER
    chains, updates banked, no gamma jumps -- engine vs oracle, generation by generation.

    Floats: epsilon = 1e-4 here, and the jitter is a float32 Box-Muller on both sides (1e-5 * epsilon = 1e-9 absolute apart: _check_generation), which
    is this test's state tolerance; the ln-likes get _check_generation's allowance for that state difference (1e3 * 1e-9).  alpha = exp(ll_prop - ll_cur)
    carries the ABSOLUTE error of that difference as its RELATIVE error: rtol = max(1e-8, twice the ln-like allowance) against the oracle -- and, free
    of the jitter, 1e-12 against the same formula (samplers.py:328-332) over the engine's own ln-likes."""
    if tgt == "banana":
        tid, params = R.TARGET_BANANA_2D, R.banana_params()
    elif tgt == "mix":
        tid, params = R.TARGET_MIXTURE_PAIRS, _mix_params()
    else:
        tid, params = R.TARGET_GAUSS_EQUICORR, _gauss_params(d)
    eng, ora = _pair_traced(R.ALGO_DEMC_SYNC, N, d, tid, params, 31)
    rs = np.random.RandomState(6)
    X = rs.normal(size=(N, d)) + 0.3
    if tgt == "mix":
        X = np.where(rs.uniform(size=(N, 1)) < 0.3, 0.0, 2.0) + 0.3 * rs.normal(size=(N, d))
    eng.set_state(X); ora.set_state(X)
    eng.set_trace(True)
    gamma = 0.7 if d <= 100 else 2.38 / np.sqrt(2.0 * d)        # (the wide rows: demc.py:162's own scale, or nothing is ever accepted there)
    eng.begin_run(epsilon=1e-4, gamma=gamma, shuffle=False, flip=0.0)
    ora.local_n_accepted, ora.local_n_rejected = 0, 1
    atol_state = 1e-9                                      # epsilon = 1e-4 float32 jitter
    atol_ll = max(1e-12, 1e3 * atol_state)
    n_acc = 0
    ll_prev = eng.get_loglike()
    np.testing.assert_allclose(ll_prev, ora.ll, rtol=RTOL_STEP, atol=1e-12)
    for g in range(12):
        ora.trace = []
        eng.step(1)
        ora._generation(g, 0.0, False, 1e-4, 1e-2, gamma)
        tr = eng.get_trace()
        assert np.array_equal(tr["partners"][:, 0], ora.trace[-1]["pa"]) and np.array_equal(tr["partners"][:, 1], ora.trace[-1]["pb"])
        assert np.all(tr["partners"][:, 0] != np.arange(N)) and np.all(tr["partners"][:, 1] != np.arange(N))
        assert np.all(tr["partners"][:, 0] != tr["partners"][:, 1])
        assert np.array_equal(tr["accepted"].astype(bool), ora.trace[-1]["accepted"])
        assert not tr["jump"].any()
        np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-12, atol=1e-9)     # epsilon = 1e-4 float32 jitter
        ll_now = eng.get_loglike()
        err_ll = float(np.max(np.abs(ll_now - ora.ll)))
        err_lp = float(np.max(np.abs(tr["ll_prop"] - ora.trace[-1]["ll_prop"])))
        with np.errstate(divide="ignore", invalid="ignore"):
            err_al = float(np.nanmax(np.abs(tr["alpha"] - ora.trace[-1]["alpha"]) / ora.trace[-1]["alpha"]))
        print("generation %d: max |ll - oracle| %.3e, |ll_prop - oracle| %.3e, alpha relative %.3e" % (g, err_ll, err_lp, err_al))
        np.testing.assert_allclose(ll_now, ora.ll, rtol=RTOL_STEP, atol=atol_ll)
        np.testing.assert_allclose(tr["ll_prop"], ora.trace[-1]["ll_prop"], rtol=RTOL_STEP, atol=atol_ll)
        np.testing.assert_allclose(tr["alpha"], ora.trace[-1]["alpha"], rtol=max(1e-8, 2.0 * atol_ll), atol=1e-300)
        np.testing.assert_allclose(tr["alpha"], R.mut_prop_ratio(ll_prev, tr["ll_prop"]), rtol=1e-12, atol=1e-300)
        # an accepted chain's ln-like is its proposal's, a rejected one keeps its own (the banana's lean form re-evaluates it from the row on demand)
        np.testing.assert_allclose(ll_now, np.where(tr["accepted"].astype(bool), tr["ll_prop"], ll_prev), rtol=RTOL_STEP, atol=1e-12)
        ll_prev = ll_now
        n_acc += int(np.count_nonzero(ora.trace[-1]["accepted"]))
    assert 0 < n_acc < 12 * N                              # both branches ran: accepted, and banked unchanged
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted and st["history_rows"] == 13
    np.testing.assert_allclose(eng.get_history(), ora.history_array(), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(eng.get_loglike_history(), np.stack(ora.ll_history), rtol=RTOL_STEP, atol=atol_ll)


def test_gpu_reproduces_committed_engine_fixture(golden_dir):
    """The HIP path against the COMMITTED fixture tests/golden/engine_layout_v3.npz (no oracle call at all):
    device-side init jitter, DREAM with adaptation, DE-MC with snooker, synchronous DE-MC."""
    g = np.load(os.path.join(golden_dir, "engine_layout_v3.npz"))
    e = _engine(algo=R.ALGO_DREAM, n_chains=12, dim=6, target_id=R.TARGET_GAUSS_EQUICORR, target_params=_gauss_params(6),
                seed=2024, burnin_gen=6, n_cr_gen=2)
    e.init_chains(np.linspace(-1, 1, 6), 1e-2)
    e.begin_run(); e.step(10)
    np.testing.assert_allclose(e.get_state(), g["dream_state"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(e.stats()["p_cr"], g["dream_p_cr"], rtol=1e-8)
    assert e.stats()["local_n_accepted"] == int(g["dream_acc"][0])
    e = _engine(algo=R.ALGO_DEMC, n_chains=9, dim=2, target_id=R.TARGET_BANANA_2D, target_params=R.banana_params(), seed=2025,
                p_snooker=0.3)
    e.init_chains(np.zeros(2), 1e-1)
    e.begin_run(); e.step(12)
    np.testing.assert_allclose(e.get_state(), g["demc_state"], rtol=1e-10, atol=1e-13)
    assert e.stats()["local_n_accepted"] == int(g["demc_acc"][0])
    e = _engine(algo=R.ALGO_DEMC_SYNC, n_chains=8, dim=3, target_id=R.TARGET_GAUSS_EQUICORR, target_params=_gauss_params(3), seed=2026)
    e.init_chains(np.zeros(3), 1e-1)
    e.begin_run(epsilon=1e-3); e.step(12)
    np.testing.assert_allclose(e.get_state(), g["sync_state"], rtol=1e-9, atol=1e-8)
    assert e.stats()["local_n_accepted"] == int(g["sync_acc"][0])


# ------------------------------------------------------------------ host-callback path against the oracle itself
@pytest.mark.parametrize("algo,d,N,kw", [
    (R.ALGO_DREAM, 10, 16, dict(burnin_gen=6, n_cr_gen=2)),
    (R.ALGO_DREAM, 7, 12, dict(burnin_gen=0, del_pairs=2)),
    (R.ALGO_DREAM, 100, 64, dict(burnin_gen=5, n_cr_gen=1)),
    (R.ALGO_DEMC, 2, 24, dict(p_snooker=0.3)),
    (R.ALGO_DEMC, 3, 10, dict()),
    (R.ALGO_DREAM, 600, 12, dict(burnin_gen=5, n_cr_gen=1)),         # 16 coordinates per lane
    (R.ALGO_DREAM, 1201, 10, dict(burnin_gen=4, n_cr_gen=1)),        # 32 coordinates per lane, odd d
    (R.ALGO_DEMC, 2000, 8, dict(p_snooker=0.3)),
    # synchronous DE-MC, what DeMc(python_callable) drives: ONE propose / commit round per generation, the commit kernels' x_next branch (kernels.h at
    # d = 3, 100, 200; phase_wide_commit_kernel at 600 and 1201, odd d)
    (R.ALGO_DEMC_SYNC, 3, 10, dict()),
    (R.ALGO_DEMC_SYNC, 100, 24, dict()),
    (R.ALGO_DEMC_SYNC, 200, 12, dict()),
    (R.ALGO_DEMC_SYNC, 600, 12, dict()),
    (R.ALGO_DEMC_SYNC, 1201, 10, dict()),
])
def test_propose_commit_path_against_oracle(algo, d, N, kw):
    """The propose / commit kernels (arbitrary Python ln_like_fn: samplers.py:36-43) compared with OracleSampler(ll_fn=...)
    DIRECTLY -- not through the fused kernels: same callable on both sides, so every accept decision is bit-exact and the
    state differs only by the proposal arithmetic's rounding (1e-12)."""
    params = _gauss_params(d, rho=0.4)

    def py_ll(theta):
        return float(R.ll_gauss_equicorr(theta, params))

    eng = _engine(algo=algo, n_chains=N, dim=d, target_id=R.TARGET_HOST, target_params=None, seed=77, **kw)
    okw = {k: v for k, v in kw.items() if k in ("del_pairs", "burnin_gen", "n_cr_gen", "p_snooker")}
    ora = R.OracleSampler(algo, N, d, R.TARGET_HOST, None, 77, ll_fn=py_ll, **okw)
    X0 = np.random.RandomState(4).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0)
    eng.set_state(X0)
    eng.set_loglike(np.array([py_ll(x) for x in X0]))
    ora.set_state(X0)
    eng.begin_run()
    n_gens = 9
    prev = X0
    sync = algo == R.ALGO_DEMC_SYNC
    n_acc = 0
    for g in range(n_gens):
        ora.trace = []
        for ph in range(1 if sync else 2):
            props, ids = eng.propose()
            if sync:
                assert np.array_equal(ids, np.arange(N))          # every chain proposes, in chain order (samplers.py:268)
            eng.commit(np.array([py_ll(p) for p in props]))
        # the oracle's generation g of the same run (k restarts at 0 in run(): drive _generation directly)
        ora._generation(g, 0.5, True, 1e-12 if algo == R.ALGO_DREAM else 1e-15, 1e-2, None)
        tr = ora.trace[0]
        acc_o = np.zeros(N, dtype=bool)
        if sync:                                                  # _generation_sync's trace: one round, every chain
            acc_o[:] = tr["accepted"]
            assert np.all(tr["pa"] != np.arange(N)) and np.all(tr["pb"] != np.arange(N)) and np.all(tr["pa"] != tr["pb"])
        else:
            for phn in ("phase0", "phase1"):
                acc_o[tr[phn]["ids"]] = tr[phn]["accepted"]
        n_acc += int(np.count_nonzero(acc_o))
        now = eng.get_state()
        changed = np.any(now != prev, axis=1)        # (against the ENGINE's previous state: a snooker proposal of a wide row differs from the
        prev = now                                   #  oracle's in the last bits -- another summation order of its dot products)
        # a chain moved iff the oracle accepted it (proposals differ from the current state with probability 1)
        assert np.array_equal(changed, acc_o), g
        np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(eng.get_loglike(), ora.ll, rtol=1e-11, atol=1e-12)
    assert 0 < n_acc < n_gens * N                                 # accepted updates and unchanged rows both went through the commit kernel
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected
    if algo == R.ALGO_DREAM:
        np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)
        np.testing.assert_allclose(st["n_cr_updates"], ora.cr.n_cr_updates, rtol=0)
    np.testing.assert_allclose(eng.get_history(), ora.history_array(), rtol=1e-11, atol=1e-13)
    if sync:
        np.testing.assert_allclose(eng.get_loglike_history(), np.stack(ora.ll_history), rtol=1e-11, atol=1e-12)


# ------------------------------------------------------------------ ln_like_fn as HIP source (bpm_set_device_likelihood) against the oracle
GAUSS_EQUICORR_HIP = """
__device__ double ln_like(const double* x, int d, const double* p) {      // p = [rho, c0, a, b, 1/sigma ...] (oracle/sampler_ref.py: ll_gauss_equicorr)
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < d; ++j) { const double z = x[j] * p[4 + j]; s1 += z; s2 += z * z; }
    return p[1] - 0.5 * (p[2] * s2 - p[3] * s1 * s1);
}
"""


GAUSS_EQUICORR_HIP_TERMS = """
#define BPM_LN_LIKE_TERMS 2
__device__ void ln_like_terms(double xj, int j, int d, const double* p, double* acc) { const double z = xj * p[4 + j]; acc[0] += z; acc[1] += z * z; }
__device__ double ln_like_finish(const double* acc, int d, const double* p) { return p[1] - 0.5 * (p[2] * acc[1] - p[3] * acc[0] * acc[0]); }
"""


@pytest.mark.parametrize("fused", [True, False, "terms"])
@pytest.mark.parametrize("algo,d,N,kw", [
    (R.ALGO_DREAM, 10, 16, dict(burnin_gen=6, n_cr_gen=2)),
    (R.ALGO_DREAM, 100, 64, dict(burnin_gen=5, n_cr_gen=1)),
    (R.ALGO_DREAM, 100, 1000, dict(burnin_gen=3, n_cr_gen=1)),
    (R.ALGO_DREAM, 7, 501, dict(burnin_gen=0, del_pairs=2)),
    (R.ALGO_DREAM, 30, 77, dict(burnin_gen=4, n_cr_gen=2, del_pairs=1)),
    (R.ALGO_DEMC, 2, 24, dict(p_snooker=0.3)),
    (R.ALGO_DEMC, 2, 3000, dict()),
    (R.ALGO_DREAM, 8, 700, dict(burnin_gen=6, n_cr_gen=1, outlier_every=2)),        # 4 lanes per chain, history in shuffle order, the outlier check due
    (R.ALGO_DEMC, 150, 40, dict(p_snooker=0.2)),
    (R.ALGO_DEMC_SYNC, 3, 10, dict()),
    (R.ALGO_DREAM, 600, 12, dict(burnin_gen=5, n_cr_gen=1)),
    (R.ALGO_DEMC_SYNC, 100, 24, dict()),                 # synchronous DE-MC on the wide rows: one wavefront per chain, fused ...
    (R.ALGO_DEMC_SYNC, 300, 12, dict()),                 # ... four pairs per lane ...
    (R.ALGO_DEMC_SYNC, 600, 12, dict()),                 # ... and the looped kernel: never fused (d > 512), the three-kernel form with x_next
])
def test_hip_source_likelihood_against_oracle(algo, d, N, kw, fused, monkeypatch):
    """Round 5: the caller's likelihood written as HIP source, compiled with hiprtc into a kernel between the proposal and the commit kernel, the
    sampler driven by bpm_step (no host code inside a generation) -- in both forms: the update kernel itself compiled around the likelihood (fused: one
    launch per half generation) and the proposal / likelihood / commit kernels -- against OracleSampler(ll_fn = the same formula in NumPy): accept counts equal,
    state / ln-like / whole history to 1e-11 (the summation order of the two formulas differs), CR statistics to 1e-9.  Several step calls, a state
    rewritten from the host in between (bpm_refresh_device_loglike)."""
    params = _gauss_params(d, rho=0.4)

    def py_ll(theta):
        return float(R.ll_gauss_equicorr(theta, params))

    eng = _engine(algo=algo, n_chains=N, dim=d, target_id=R.TARGET_HOST, target_params=None, seed=78, **kw)
    okw = {k: v for k, v in kw.items() if k in ("del_pairs", "burnin_gen", "n_cr_gen", "p_snooker", "outlier_every")}
    ora = R.OracleSampler(algo, N, d, R.TARGET_HOST, None, 78, ll_fn=py_ll, **okw)
    X0 = np.random.RandomState(5).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0)
    eng.set_state(X0)
    with pytest.raises(Exception, match="bpm_propose / bpm_commit"):
        eng.begin_run()
        eng.step(1)                                     # (a host-callback sampler without a device likelihood cannot be stepped)
    with pytest.raises(Exception, match="does not compile"):
        eng.set_device_likelihood("__device__ double ln_like(const double* x) { return x[0] }")
    monkeypatch.setenv("BPM_USER_FUSED", "1" if fused else "0")
    # "terms": the per-coordinate form of the same likelihood (every lane of a chain adds its own coordinates' terms inside the update kernel)
    eng.set_device_likelihood(GAUSS_EQUICORR_HIP_TERMS if fused == "terms" else GAUSS_EQUICORR_HIP, params)
    is_fused, why = eng.device_likelihood_info()
    # fused: the update kernel itself compiled around the likelihood (one launch per half generation); else proposal / likelihood / commit kernels
    assert is_fused == (bool(fused) and d <= 512), why
    np.testing.assert_allclose(eng.get_loglike(), [py_ll(x) for x in X0], rtol=1e-12, atol=1e-12)
    ora.set_state(X0)
    eng.begin_run()
    g = 0
    for k in (1, 4, 2):
        eng.step(k)
        for _ in range(k):
            ora._generation(g, 0.5, True, 1e-12 if algo == R.ALGO_DREAM else 1e-15, 1e-2, None)
            g += 1
        np.testing.assert_allclose(eng.get_state(), ora.X, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(eng.get_loglike(), ora.ll, rtol=1e-11, atol=1e-12)
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected
    if algo == R.ALGO_DREAM:
        np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)
        np.testing.assert_allclose(st["n_cr_updates"], ora.cr.n_cr_updates, rtol=0)
    np.testing.assert_allclose(eng.get_history(), ora.history_array(), rtol=1e-11, atol=1e-13)
    # a state rewritten from the host: the ln-likes come from the device likelihood again
    X1 = eng.get_state() + 0.125
    eng.set_state(X1)
    eng.refresh_device_loglike()
    np.testing.assert_allclose(eng.get_loglike(), [py_ll(x) for x in X1], rtol=1e-12, atol=1e-12)
    eng.close()


# ------------------------------------------------------------------ the outlier check's device-side selection
@pytest.mark.parametrize("N", [4, 7, 100, 4097, 262144])
def test_outlier_quartile_selection_equals_numpy(N):
    """The multi-workgroup radix select + first-argmax of the outlier check against np.percentile / np.argmax on inputs a real run
    can produce: ties, chains outside a prior's support (ln-like = -inf), signed zeros, all chains equal, a wide dynamic range."""
    import ctypes as C
    from bipymc_amd import _lib as L
    eng = _hooks_engine(algo=R.ALGO_DREAM, n_chains=N, dim=2, target_id=R.TARGET_MIXTURE_PAIRS, target_params=_mix_params(), seed=1,
                        outlier_every=5)
    rs = np.random.RandomState(N)
    cases = [rs.normal(size=N) * 10 - 20,
             np.round(rs.normal(size=N) * 3),                                   # many ties
             np.where(rs.uniform(size=N) < 0.3, -np.inf, rs.normal(size=N)),    # a third of the chains at -inf
             np.where(rs.uniform(size=N) < 0.5, 0.0, -0.0),                     # signed zeros
             np.full(N, -3.25),                                                 # everybody equal
             -np.exp(rs.uniform(-40, 40, size=N)),                              # 35 orders of magnitude
             np.sort(rs.normal(size=N))[::-1].copy()]                           # descending
    for om in cases:
        om = np.ascontiguousarray(om, dtype=np.float64)
        out = np.zeros(6)
        L.check(eng.lib.bpm_debug_outlier_select(eng._h, om.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))), eng.lib)
        srt = np.sort(om)
        k0, k1 = int(np.floor(0.25 * (N - 1))), int(np.floor(0.75 * (N - 1)))
        exp = [srt[k0], srt[min(k0 + 1, N - 1)], srt[k1], srt[min(k1 + 1, N - 1)]]
        assert np.array_equal(out[:4], exp), (N, out[:4], exp)                   # (0.0 == -0.0: either sign is the same order statistic)
        assert int(out[4]) == int(np.argmax(om))                                # the FIRST maximum
        with np.errstate(invalid="ignore"):
            q1, q3 = np.percentile(om, [25.0, 75.0])
            cut = q1 - 2.0 * (q3 - q1)
        assert (np.isnan(cut) and np.isnan(out[5])) or out[5] == cut, (N, out[5], cut)
