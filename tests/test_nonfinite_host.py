"""CPU preconditions of tests/test_gpu_nonfinite.py: the oracle alone on every case of tests/_nonfinite_cases.py.  The GPU tests compare the kernels'
Metropolis step (samplers.py:328-336) with the oracle on ln-likes of -inf, NaN and +inf; they say something only while the oracle's run really goes
through those branches.  A seed or a shape that stops doing so fails here, without a GPU."""
import os
import sys

import numpy as np
import pytest

from oracle import sampler_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _nonfinite_cases as NF  # noqa: E402

_BOX = [(c[0], v) for c in NF.BOX_CASES + NF.DEVICE_CASES for v in NF.VARIANTS]


def test_the_likelihood_forms_agree_on_the_host():
    """the per-row callable against a direct restatement; the parameter block both HIP forms index"""
    for d in (3, 10, 101):
        for variant in NF.VARIANTS:
            ll = NF.BoxLikelihood(d, variant)
            X = NF.start_state(d, 64, d, every=3)
            z = X / NF.sigma_of(d)
            out = np.any(np.abs(z) > NF.bound_of(d), axis=1)
            want = R.ll_gauss_equicorr(X, R.gauss_equicorr_params(NF.RHO, NF.sigma_of(d)))
            if variant == "bands":
                want = np.where(X[:, 0] < -2.0, np.nan, want)
                want = np.where(X[:, 0] > 2.0, np.inf, want)
            want = np.where(out, -np.inf, want)
            got = ll.rows(X)
            assert 0 < np.count_nonzero(out) < 64
            NF.assert_same_classes_and_close(got, want, rtol=1e-13, atol=0)
            assert ll.params.size == 4 + d + 3 and ll.params[4 + d] == NF.bound_of(d) and ll.params[5 + d] == -2.0 and ll.params[6 + d] == 2.0


def test_hip_sources_take_the_forms_the_issue_names():
    for variant in NF.VARIANTS:
        src, k = NF.hip_source(variant, terms=False)
        assert k == 0 and "ln_like(" in src and "BPM_LN_LIKE_TERMS" not in src
        src, k = NF.hip_source(variant, terms=True)
        assert k == (4 if variant == "bands" else 3) and "#define BPM_LN_LIKE_TERMS %d" % k in src and "ln_like_finish" in src


@pytest.mark.parametrize("name,variant", _BOX, ids=["%s-%s" % t for t in _BOX])
def test_oracle_goes_through_every_branch_on_the_box(name, variant):
    r = NF.oracle_box_run(name, variant)
    n_from_minf = int(sum(np.count_nonzero(m) for m in r.from_minf))
    print("%s %s: n_nan %d, accepted %d, rejected %d, accepted from -inf %d, margin %.3g, resets %d, p_cr %s" %
          (name, variant, r.n_nan[-1], r.n_acc[-1], r.n_rej[-1], n_from_minf, r.margin, r.resets[-1], r.p_cr[-1]), r.n_returned)
    assert r.n_nan[-1] > 0                                    # NaN alphas: both ln-likes -inf (or a NaN / two +inf in "bands")
    assert n_from_minf >= 1                                   # ll_cur = -inf, proposal inside: alpha = +inf clipped to 1, the chain returns
    assert 0 < r.n_acc[-1] < NF.GENS * r.N
    assert r.margin >= NF.MARGIN, r.margin                    # no proposal so close to a face that oracle and kernel could classify it differently
    assert np.all(np.isfinite(r.p_cr[-1]))
    assert np.all(np.isfinite(r.history))                     # (the STATES stay finite: only ln-likes are not)
    nan_, pinf, minf = NF.value_classes(r.ll_history)
    assert minf.any()
    if variant == "bands":                                    # all four value classes in one run: every one came out of the likelihood
        assert all(n > 0 for n in r.n_returned.values()), r.n_returned
        assert np.isfinite(r.ll_history).any()
    else:
        assert r.n_returned["nan"] == 0 and r.n_returned["pinf"] == 0 and not nan_.any() and not pinf.any()
    if "outlier_every" in r.kw:
        # N = 40, every 13th chain outside: the chains at -inf are the ones reset; N = 700, every fourth: the quartiles are not finite, no reset
        assert (r.resets[-1] > 0) == (r.N == 40), r.resets


@pytest.mark.parametrize("case", NF.OVERFLOW_CASES, ids=NF.OVERFLOW_IDS)
def test_oracle_on_the_shipped_targets_from_overflow_rows(case):
    algo, N, d, tid, params, seed, X0, kw, _launches = NF.overflow_case(*case)
    ora = R.OracleSampler(algo, N, d, tid, params, seed, **kw)
    with np.errstate(all="ignore"):
        ora.set_state(X0)
        ll0 = ora.ll.copy()
        ora.run(NF.OVERFLOW_GENS)
    print("%s: n_nan %d, accepted %d, rejected %d, ll of the overflow rows %s" % (case, ora.n_nan, ora.local_n_accepted, ora.local_n_rejected, ll0[[1, 5]]))
    assert not np.isfinite(ll0[1]) and not np.isfinite(ll0[5]) and np.all(np.isfinite(np.delete(ll0, [1, 5])))
    if case[1] == "banana" or (case[1] == "gauss" and params[0] == 0.0):
        # (the Gaussian at rho = 0: b = 0 and b * s1 * s1 = (0 * s1) * s1 = 0, so ll = c0 - 0.5 * a * inf)
        assert ll0[1] == -np.inf and ll0[5] == -np.inf
    else:
        assert np.isnan(ll0[1]) and np.isnan(ll0[5])
    assert ora.n_nan > 0 and ora.local_n_accepted > 0
    H = ora.history_array()
    others = np.delete(np.arange(N), [1, 5])
    assert np.all(np.isfinite(H[:, others]))                   # every history stays finite except the two chains' own rows
    assert np.all(H[:, [1, 5]] == X0[[1, 5]])                  # ... which never move
    assert np.all(np.isfinite(np.stack(ora.ll_history)[:, others]))
    if algo == R.ALGO_DREAM:
        assert np.all(np.isfinite(ora.cr.p_cr))                # (burnin_gen = 0: no adaptation, p_cr stays uniform)
