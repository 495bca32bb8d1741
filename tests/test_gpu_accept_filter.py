"""The accept test of the update kernels (bipymc_amd/csrc/accept_test.h) on the device: a float32 2^t -- one v_exp_f32 -- decides u < clip(exp(d), 0, 1)
wherever u lies outside its error margin DELTA = 2^-12, the plain formula (the device library's f64 exp) behind a branch everywhere else.

a. bpm_selftest_accept (test variant): every decision and NaN flag against the plain formula evaluated beside it on the device, for the input classes
   of tests/test_accept_filter_host.py -- zero differences, and the exact path taken for some cases but not all.
b. bpm_selftest_accept_error: the measured relative error of the float32 route -- every float t in [-58, -2^-20] against the library's f64 exp2, and 10^6
   doubles d in [D_LO, 0) through the whole route against the library's exp(d).  Both maxima must stay under DELTA / 16: the margin's design condition
   (accept_test.h derives 2.6e-6 = DELTA / 94 from v_exp_f32's 1 ulp), not a tuning number.
c. 12 generations (k = 0, 5, 10: the gamma = 1 jumps of dream.py:77-80 / demc.py:174-177, where d << D_LO) on the smallest shapes that reach every copy
   of the accept test, against the CPU oracle with the helpers of tests/test_gpu_shipped_path.py and tests/test_gpu_parity.py.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import sampler_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

D_LO, DELTA = -40.0, 2.0 ** -12          # accept_test.h: ACCEPT_D_LO, ACCEPT_DELTA
GENS = 12


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _cases():
    """(d, u, adversarial) -- d: the special values and 10^6 random ones in [-45, 1]; u: {0, 2^-53, 1 - 2^-53}, a random 53-bit value, and the five
    doubles within +-2 ulp of the clamped exp(d)"""
    rs = np.random.RandomState(20261019)
    special = np.array([0.0, -0.0, 1e-300, -1e-300, D_LO, np.nextafter(D_LO, -np.inf), np.nextafter(D_LO, np.inf), -745.0, -746.0, -1e300,
                        np.inf, -np.inf, np.nan])
    d = np.concatenate([special, -45.0 + 46.0 * rs.random_sample(1000000)])
    with np.errstate(all="ignore"):
        a = np.clip(np.minimum(1.0, np.exp(d)), 0.0, 1.0)
    a = np.where(np.isnan(a), 0.5, a)
    us, adv = [], []
    for fixed in (0.0, 2.0 ** -53, 1.0 - 2.0 ** -53):
        us.append(np.full_like(d, fixed)); adv.append(False)
    us.append(rs.randint(0, 2 ** 53, size=d.size, dtype=np.int64) * 2.0 ** -53); adv.append(False)
    lo, hi = a, a
    us.append(a); adv.append(True)
    for _ in range(2):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        us.append(lo); adv.append(True)
        us.append(hi); adv.append(True)
    D = np.ascontiguousarray(np.tile(d, len(us)))
    U = np.ascontiguousarray(np.concatenate(us))
    A = np.repeat(np.array(adv), d.size)
    return D, U, A


def test_decisions_on_the_device_equal_the_plain_formula_with_the_librarys_exp():
    from bipymc_amd import _lib as L
    lib = L.load_test()
    D, U, A = _cases()
    n = D.size
    out = [np.zeros(n, dtype=np.uint8) for _ in range(5)]
    L.check(lib.bpm_selftest_accept(0, n, _dp(D), _dp(U), *[o.ctypes.data_as(C.POINTER(C.c_uint8)) for o in out]), lib)
    acc_f, acc_e, nan_f, nan_e, exact = out
    print("cases %d  accepted %d  NaN %d  exact path %d (adversarial u: %d of %d, other u: %d of %d)"
          % (n, int(acc_e.sum()), int(nan_e.sum()), int(exact.sum()), int(exact[A].sum()), int(A.sum()), int(exact[~A].sum()), int((~A).sum())))
    bad = np.flatnonzero((acc_f != acc_e) | (nan_f != nan_e))
    assert bad.size == 0, [(float.hex(float(D[i])), float.hex(float(U[i])), int(acc_f[i]), int(acc_e[i])) for i in bad[:5]]
    assert int(nan_e.sum()) == int(np.isnan(D).sum()) > 0
    assert 0 < int(acc_e.sum()) < n
    assert 0 < int(exact.sum()) < n
    assert 0 < int(exact[A].sum()) < int(A.sum())


def test_measured_error_of_the_float32_route_is_far_inside_the_margin():
    from bipymc_amd import _lib as L
    lib = L.load_test()
    d = np.ascontiguousarray(D_LO * (1.0 - np.random.RandomState(7).random_sample(1000000)))      # (D_LO, 0) and D_LO itself
    d[0] = D_LO
    assert np.all((d >= D_LO) & (d < 0.0))
    out = np.zeros(2)
    L.check(lib.bpm_selftest_accept_error(0, d.size, _dp(d), _dp(out)), lib)
    print("max |exp2_f32(t) / exp2_f64(t) - 1| over every float t in [-58, -2^-20]: %.4g (DELTA / %.0f)" % (out[0], DELTA / out[0]))
    print("max |route(d) / exp(d) - 1| over 10^6 d in [D_LO, 0): %.4g (DELTA / %.0f)" % (out[1], DELTA / out[1]))
    assert 0.0 < out[0] <= DELTA / 16
    assert 0.0 < out[1] <= DELTA / 16


def _gauss(N, d, seed):
    sig = np.sqrt(np.arange(d) + 1.0)
    return R.TARGET_GAUSS_EQUICORR, R.gauss_equicorr_params(0.5, sig), np.random.RandomState(seed).normal(size=(N, d)) * sig


DREAM_KW = dict(del_pairs=3, n_cr=3, burnin_gen=4, n_cr_gen=2)
RUNS = {
    "dream_d100_one_wavefront_per_chain_planned_front": (R.ALGO_DREAM, 64, 100, "gauss", DREAM_KW),
    "dream_d101_planned_front_odd_dim": (R.ALGO_DREAM, 64, 101, "gauss", DREAM_KW),
    "dream_d8_four_lanes_per_chain": (R.ALGO_DREAM, 256, 8, "gauss", DREAM_KW),
    "demc_snooker_d2_one_lane_per_chain": (R.ALGO_DEMC, 1024, 2, "banana", dict(p_snooker=0.1)),
    "dream_d600_looped_wide_kernel": (R.ALGO_DREAM, 64, 600, "gauss", DREAM_KW),
    "demc_d600_looped_wide_kernel": (R.ALGO_DEMC, 64, 600, "gauss", dict(p_snooker=0.3)),
}


@pytest.mark.parametrize("case", sorted(RUNS))
def test_short_runs_on_every_copy_of_the_accept_test_equal_the_oracle(case):
    from test_gpu_shipped_path import _run_both
    algo, N, d, tgt, kw = RUNS[case]
    if tgt == "banana":
        tid, params, X0 = R.TARGET_BANANA_2D, R.banana_params(), np.random.RandomState(5).normal(size=(N, 2)) + np.array([0.0, 1.0])
    else:
        tid, params, X0 = _gauss(N, d, 100 + d)
    if d > 512:
        _run_wide(algo, N, d, tid, params, X0, kw)
    else:
        _run_both(algo, N, d, tid, params, 42, X0, GENS, kw, hist_rows=(5, GENS))


def _run_wide(algo, N, d, tid, params, X0, kw):
    """the looped wide-row kernel against the oracle, compared as tests/test_gpu_shipped_path.py compares it
    (test_looped_wide_row_kernel_on_the_shipped_path_equals_the_oracle: its tolerances, for the reasons given there), over GENS generations"""
    from bipymc_amd.engine import HipEngine
    from test_gpu_shipped_path import ATOL, RTOL
    eng = HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=params, seed=42, **kw)
    ora = R.OracleSampler(algo, N, d, tid, params, 42, **kw)
    eng.set_state(X0)
    ora.set_state(X0)
    ls0 = eng.launch_stats()
    eng.begin_run()
    eng.step(GENS)
    eng.synchronize()
    ora.run(GENS)
    ls = eng.launch_stats()
    assert ls["direct"] - ls0["direct"] == 2 * GENS and ls["stream"] == ls0["stream"], (ls0, ls)
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected
    assert st["n_nan_alpha"] == ora.n_nan == 0
    np.testing.assert_allclose(eng.get_state(), ora.X, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(eng.get_history(), np.stack(ora.history, axis=0), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(eng.get_loglike(), ora.ll, rtol=1e-9, atol=1e-7)
    if algo == R.ALGO_DREAM:
        np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-7)
        assert np.array_equal(st["n_cr_updates"], ora.cr.n_cr_updates)
    eng.close()


def test_host_callback_run_through_propose_and_commit_equals_the_oracle():
    """phase_commit_kernel's copy (finish_update behind bpm_propose / bpm_commit): the same Python ln_like on both sides, so every accept decision is
    the oracle's and the state differs by the proposal arithmetic's rounding only (tests/test_gpu_parity.py: test_propose_commit_path_against_oracle)."""
    from test_gpu_parity import _engine, _gauss_params
    N, d, kw = 64, 100, dict(burnin_gen=5, n_cr_gen=1)
    params = _gauss_params(d, rho=0.4)

    def py_ll(theta):
        return float(R.ll_gauss_equicorr(theta, params))

    eng = _engine(algo=R.ALGO_DREAM, n_chains=N, dim=d, target_id=R.TARGET_HOST, target_params=None, seed=77, **kw)
    ora = R.OracleSampler(R.ALGO_DREAM, N, d, R.TARGET_HOST, None, 77, ll_fn=py_ll, **kw)
    X0 = np.random.RandomState(4).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0)
    eng.set_state(X0)
    eng.set_loglike(np.array([py_ll(x) for x in X0]))
    ora.set_state(X0)
    eng.begin_run()
    prev, n_acc = X0, 0
    for g in range(GENS):
        ora.trace = []
        for _ph in range(2):
            props, _ids = eng.propose()
            eng.commit(np.array([py_ll(p) for p in props]))
        ora._generation(g, 0.5, True, 1e-12, 1e-2, None)
        acc_o = np.zeros(N, dtype=bool)
        for phn in ("phase0", "phase1"):
            acc_o[ora.trace[0][phn]["ids"]] = ora.trace[0][phn]["accepted"]
        n_acc += int(np.count_nonzero(acc_o))
        now = eng.get_state()
        assert np.array_equal(np.any(now != prev, axis=1), acc_o), g      # a chain moved iff the oracle accepted it
        prev = now
        np.testing.assert_allclose(now, ora.X, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(eng.get_loglike(), ora.ll, rtol=1e-11, atol=1e-12)
    assert 0 < n_acc < GENS * N
    st = eng.stats()
    assert st["local_n_accepted"] == ora.local_n_accepted and st["local_n_rejected"] == ora.local_n_rejected and st["n_nan_alpha"] == 0
    np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)
    np.testing.assert_allclose(eng.get_history(), ora.history_array(), rtol=1e-11, atol=1e-13)
    eng.close()
