"""The update kernels reproduce, BIT FOR BIT, what the library of the commit before the reductions were re-scheduled computed
(tests/golden/update_bits.json, written on the GPU by tools/update_bits.py from that commit's library).

The sums of the update kernels keep their tree -- lanes at distance 1, 2, the half-mirror, the mirror of a row of 16 lanes, then the rows
(0 + 1) + (2 + 3) -- whatever lanes and instructions carry it (bipymc_amd/csrc/kernels.h: gsum, gsum2, row_sums_f64); the Philox words are
the same whichever bitwise instruction mixes them.  The oracle's 1e-12 would not notice another association; SHA-256 digests of the state,
the ln-likes, the whole history, p_cr and the CR statistics, and the accept counts do.

Cases (tools/update_bits.py: cases): N = 128 chains, 12 generations, fixed seeds;
  DREAM adapting throughout (the 1024-thread burn-in flavour) and in steady state at d = 100, 34 (rows 2 and 3 of the wavefront are padding:
  the row combine adds their zeros in place), 127 (odd, every lane live), 32, 8, 2 (16, 4, 1 lanes per chain); DE-MC with snooker updates at
  d = 100 and 2; the looped wide-row kernel at d = 640; and d = 100 from a start whose ln-like sums change in their last bits under any other
  association (coordinates 0, 2, 4, ... alternate +-1e8, the others are of order 1).  Seed of that start and of its sampler: 11
  (tools/update_bits.py: ASSOC_SEED); the CPU test below checks with the oracle that it yields finite ln-likes and accepted updates
  (750 of 1536 in 12 generations)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import update_bits as U      # noqa: E402

_CASES = U.cases()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "update_bits.json")) as f:
        return json.load(f)


def test_golden_file_holds_every_case(golden):
    assert golden["n_chains"] == U.N_CHAINS and golden["n_gens"] == U.N_GENS
    assert sorted(golden["cases"]) == sorted(c[0] for c in _CASES)
    # every case moved: a digest of a run in which nothing was accepted would compare nothing
    for name, c in golden["cases"].items():
        assert c["n_accepted"] > 0 and c["history_rows"] == U.N_GENS + 1, (name, c)


def test_association_order_start_is_finite_and_moves_on_the_oracle():
    """oracle/sampler_ref.py on the association-order start: finite ln-likes throughout and accepted updates, with seed ASSOC_SEED"""
    from oracle import sampler_ref as R
    d = 100
    assert np.array_equal(U.gauss_params(d), R.gauss_equicorr_params(0.5, np.sqrt(np.arange(d) + 1.0)))
    X0 = U.assoc_state(d, U.ASSOC_SEED)
    assert np.all(np.abs(X0[:, 0::2]) > 9e7) and np.all(np.abs(X0[:, 1::2]) < 10.0)
    ora = R.OracleSampler(R.ALGO_DREAM, U.N_CHAINS, d, R.TARGET_GAUSS_EQUICORR, U.gauss_params(d), U.ASSOC_SEED, burnin_gen=0)
    ora.set_state(X0)
    ora.run(U.N_GENS)
    assert np.all(np.isfinite(np.array(ora.ll_history))) and np.all(np.isfinite(ora.ll))
    print("accepted", ora.local_n_accepted, "of", ora.local_n_accepted + ora.local_n_rejected - 1)
    assert ora.local_n_accepted > 0
    # the sums really are order-sensitive there: two orders of the same additions differ
    z = X0[0] * U.gauss_params(d)[4:]
    assert float(np.sum(z * z)) != float(np.sum((z * z)[::-1])) or float(np.sum(z)) != float(np.sum(z[::-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_update_kernels_reproduce_the_parent_commits_bits(case, golden):
    name, algo, d, kw, X0 = case
    got = U.run_case(algo, d, kw, X0)
    want = golden["cases"][name]
    print(name, "accepted", got["n_accepted"], "rejected", got["n_rejected"])
    for key in sorted(want):
        assert got[key] == want[key], "%s: %s differs from the library of build %s" % (name, key, golden["library_build_id"])
