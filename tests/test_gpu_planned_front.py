"""The planned front of the one-wavefront-per-chain update kernels (bipymc_amd/csrc/kernels.h: plan_front) against the CPU oracle, on the path
that ships: own queue, acquire-only packets, no trace -- exactly as tests/test_gpu_shipped_path.py::_run_both compares (integers equal, floats to
rtol 1e-10 / atol 1e-12, history rows of one burn-in and one steady generation).

The front reads the whole 64-byte record and the first lines of the argument block behind one wait, requests the own row and the 2 NP partner
rows from every lane (index clamped to the row's last pair), and reads everything else behind them.  The shapes are the smallest at which such a
front can go wrong:

  d    33   smallest row the 64 x 2 shape serves: 47 lanes beyond the row, the gamma table's index clamped
       100  the headline row
       127  odd: the last lane holds one coordinate
       128  every lane full
  N    18   9 items per half generation: an idle wavefront in the last 2-wavefront workgroup, fewer items than a 16-wavefront burn-in workgroup
       70   35 items per half generation: a partial last workgroup in both block sizes

Reference arithmetic restated by the oracle: bipymc/dream.py:32-140, bipymc/demc.py:63-151,153-196, bipymc/samplers.py:328-336."""
import numpy as np
import pytest

from oracle import sampler_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-10, 1e-12


def _run_both(algo, N, d, seed, gens, okw, hist_rows):
    from bipymc_amd.engine import HipEngine
    params = R.gauss_equicorr_params(0.5, np.sqrt(np.arange(d) + 1.0))
    rs = np.random.RandomState(1000 * d + N)
    X0 = np.sqrt(np.arange(d) + 1.0) * (np.sqrt(0.5) * rs.standard_normal((N, 1)) + np.sqrt(0.5) * rs.standard_normal((N, d)))
    eng = HipEngine(algo=algo, n_chains=N, dim=d, target_id=R.TARGET_GAUSS_EQUICORR, target_params=params, seed=seed, **okw)
    ora = R.OracleSampler(algo, N, d, R.TARGET_GAUSS_EQUICORR, params, seed, **okw)
    ls0 = eng.launch_stats()
    assert ls0["has_queue"], "no direct AQL queue on this box: " + str(ls0)
    assert ls0["fence"] == "acquire" and not ls0["coherent_state"], ls0
    eng.set_state(X0)
    ora.set_state(X0)
    eng.begin_run()
    eng.step(gens)                         # NO trace: the specialised (HOT) instantiations run
    eng.synchronize()
    ls = eng.launch_stats()
    assert ls["direct"] - ls0["direct"] == 2 * gens and ls["stream"] == ls0["stream"], (ls0, ls)   # every update kernel through the own queue
    ora.run(gens)
    st = eng.stats()
    # ---- integers: exact
    assert st["local_n_accepted"] == ora.local_n_accepted, (st["local_n_accepted"], ora.local_n_accepted)
    assert st["local_n_rejected"] == ora.local_n_rejected
    assert st["n_nan_alpha"] == ora.n_nan == 0
    # ---- floats
    np.testing.assert_allclose(eng.get_state(), ora.X, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(eng.get_loglike(), ora.ll, rtol=RTOL, atol=1e-9)
    for g in hist_rows:
        np.testing.assert_allclose(eng.get_history(g, g + 1)[0], ora.history[g], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(eng.get_loglike_history(g, g + 1)[0], ora.ll_history[g], rtol=RTOL, atol=1e-9)
    if algo == R.ALGO_DREAM:
        np.testing.assert_allclose(st["p_cr"], ora.cr.p_cr, rtol=1e-9)
        np.testing.assert_allclose(st["delta_m"], ora.cr.delta_m, rtol=1e-6)        # divides by per-chain history variances: see test_gpu_parity
        assert np.array_equal(st["n_cr_updates"], ora.cr.n_cr_updates)
    eng.close()


@pytest.mark.parametrize("N", [18, 70])
@pytest.mark.parametrize("d", [33, 100, 127, 128])
def test_dream_burn_in_then_steady_state_equals_the_oracle(d, N):
    """DREAM, three pairs, three CR values: 4 burn-in generations (HOT 3, CR gate open from generation 3), then 8 steady ones (HOT 1)."""
    _run_both(R.ALGO_DREAM, N, d, 42, 12, dict(del_pairs=3, n_cr=3, burnin_gen=4, n_cr_gen=2), hist_rows=(3, 12))


def test_demc_with_two_partner_rows_equals_the_oracle():
    """DE-MC (NP = 1): the planned path with two partner rows; 11 generations, so that k = 0 and k = 10 (gamma = 1 jumps) are both inside."""
    _run_both(R.ALGO_DEMC, 18, 40, 7, 11, {}, hist_rows=(1, 11))


def test_steady_run_crosses_into_the_second_record_table():
    """Records are built per window of 64 generations: 70 steady generations cross into the second table buffer, where a record read at a
    wrong offset would show."""
    _run_both(R.ALGO_DREAM, 18, 100, 42, 70, dict(del_pairs=3, n_cr=3, burnin_gen=0, n_cr_gen=2), hist_rows=(63, 64, 65, 70))
