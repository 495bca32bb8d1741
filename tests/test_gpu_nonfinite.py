"""Every update path on ln-likelihoods that are NOT finite, against the CPU oracle.

The Metropolis step (samplers.py:328-336; oracle/sampler_ref.py: mut_prop_ratio, metropolis_accept) exists in several hand-written copies -- finish_update
(kernels.h), two places of kernels_wide.h, the commit kernels of the propose / commit path, the run-time compiled update kernel around a HIP-source
likelihood -- and around it sit paths that treat ll_cur and the accept flag differently (the lean path, the planned front, the x_next branch of
synchronous DE-MC, the accept bytes of the replay exchange, the push of accepted rows, the NaN counter's atomic).  Every other oracle-parity test runs a
smooth target from a start inside its support and asserts n_nan_alpha == 0.  Here:

  1. a bounded-support likelihood (-inf outside a box; "bands": NaN and +inf inside it too) in every form the sampler accepts -- Python callable on the
     propose / commit path, HIP source in the whole-row and the per-coordinate form (fused and as three kernels), a torch function on the device --
     from starts with chains outside the box;
  2. the shipped targets from start rows of magnitude 1e160 (z * z overflows: NaN or -inf without any user code), on the shipped path;
  3. the alternative kernel paths on those starts, bit for bit against the default path;
  4. two ranks over the push and the replay exchange on such a start, bit for bit against one rank;
  5. the trace summaries' ln-like statistics on a history with -inf, +inf and NaN in it (the sampler classes on a start with every chain outside the
     support: tests/test_gpu_api.py::test_nan_ratio_raises_on_the_device_paths_too).

What the oracle's runs contain (NaN alphas, returns from -inf, the distance of every proposal from the box's faces) is asserted without a GPU in
tests/test_nonfinite_host.py."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import sampler_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _nonfinite_cases as NF  # noqa: E402
from test_gpu_shipped_path import _run_both  # noqa: E402

CHILD_LIMIT_S = 240


def _engine(**kw):
    from bipymc_amd.engine import HipEngine
    return HipEngine(**kw)


def _check_counters(eng, r, g):
    """accept / reject / NaN-alpha counters after generation g (0-based) equal the oracle's"""
    st = eng.stats()
    assert (st["local_n_accepted"], st["local_n_rejected"]) == (r.n_acc[g], r.n_rej[g]), (g, st["local_n_accepted"], r.n_acc[g])
    assert st["n_nan_alpha"] == r.n_nan[g], (g, st["n_nan_alpha"], r.n_nan[g])
    return st


def _check_end(eng, r, st, ll_history):
    assert st["n_nan_alpha"] == r.n_nan[-1] > 0
    np.testing.assert_allclose(eng.get_history(), r.history, rtol=1e-11, atol=1e-13)
    if ll_history:
        NF.assert_same_classes_and_close(eng.get_loglike_history(), r.ll_history, 1e-11, 1e-12, "ln-like history")
    if r.algo == R.ALGO_DREAM:
        print("p_cr relative deviation from the oracle: %.3g" % np.max(np.abs(st["p_cr"] / r.p_cr[-1] - 1.0)))
        np.testing.assert_allclose(st["p_cr"], r.p_cr[-1], rtol=1e-9)            # (as both copied drivers hold it, at every shape)
        np.testing.assert_allclose(st["n_cr_updates"], r.n_cr_updates, rtol=0)


# ------------------------------------------------------------------ 1. the box, propose / commit path
_COMMIT = [(n, v) for n in NF.COMMIT_CASES for v in NF.VARIANTS]


@pytest.mark.parametrize("name,variant", _COMMIT, ids=["%s-%s" % t for t in _COMMIT])
def test_propose_commit_path_on_nonfinite_ln_likes(name, variant):
    """test_gpu_parity.py::test_propose_commit_path_against_oracle's loop with the bounded-support callable on both sides: the commit kernels (kernels.h at
    d <= 512, phase_wide_commit_kernel beyond; the x_next branch for synchronous DE-MC) decide on ln-likes of -inf (and NaN / +inf: "bands").  Per
    generation: a chain moved iff the oracle accepted it, in particular every chain that came back from ll_cur = -inf; the three counters; state and
    ln-like to that test's tolerances (1e-11 / 1e-13, 1e-12 for ln-likes), the ln-likes' NaN, +inf and -inf each at the oracle's positions."""
    r = NF.oracle_box_run(name, variant)
    assert r.margin >= NF.MARGIN, r.margin
    ll = NF.BoxLikelihood(r.d, variant)                       # (the engine's own instance: the cached oracle run's record stays as it is)
    eng = _engine(algo=r.algo, n_chains=r.N, dim=r.d, target_id=R.TARGET_HOST, target_params=None, seed=r.seed, **r.kw)
    eng.set_state(r.X0)
    eng.set_loglike(ll.rows(r.X0))
    eng.begin_run()
    prev = r.X0
    sync = r.algo == R.ALGO_DEMC_SYNC
    n_back = 0
    for g in range(NF.GENS):
        for ph in range(1 if sync else 2):
            props, ids = eng.propose()
            eng.commit(ll.rows(props))
        now = eng.get_state()
        changed = np.any(now != prev, axis=1)
        prev = now
        assert np.array_equal(changed, r.acc[g]), (g, np.nonzero(changed != r.acc[g])[0])
        assert np.all(changed[r.from_minf[g]]), g                           # ll_cur = -inf, the proposal inside the box: always accepted
        n_back += int(np.count_nonzero(r.from_minf[g]))
        st = _check_counters(eng, r, g)
        np.testing.assert_allclose(now, r.X[g + 1], rtol=1e-11, atol=1e-13)
        NF.assert_same_classes_and_close(eng.get_loglike(), r.ll[g + 1], 1e-11, 1e-12, "ln-likes after generation %d" % g)
    assert n_back >= 1
    _check_end(eng, r, st, ll_history=True)
    eng.close()


# ------------------------------------------------------------------ 1. the box as HIP source
_HIP = [(c[0], v) for c in NF.BOX_CASES for v in NF.VARIANTS]


@pytest.mark.parametrize("fused", [True, False, "terms"])
@pytest.mark.parametrize("name,variant", _HIP, ids=["%s-%s" % t for t in _HIP])
def test_hip_source_likelihood_on_nonfinite_ln_likes(name, variant, fused, monkeypatch):
    """test_gpu_parity.py::test_hip_source_likelihood_against_oracle's loop (bpm_step drives; several step calls) with the bounded-support likelihood as
    HIP source: the update kernel compiled around it (fused: the whole-row form on one lane per chain, "terms": every lane adds its coordinates' terms and
    a third accumulator counts coordinates outside the box), and the proposal / likelihood / commit kernels (d > 512 is never fused).  After every
    step call: the accept decisions of its generations (who moved), the three counters, state and ln-likes (tolerances of that test; NaN / +inf / -inf each at the oracle's positions); at the end the
    histories, the CR statistics and the outlier resets (N = 40: the chains at -inf are the ones reset; N = 700: the quartiles are not finite, none)."""
    r = NF.oracle_box_run(name, variant)
    assert r.margin >= NF.MARGIN, r.margin
    eng = _engine(algo=r.algo, n_chains=r.N, dim=r.d, target_id=R.TARGET_HOST, target_params=None, seed=r.seed, **r.kw)
    eng.set_state(r.X0)
    monkeypatch.setenv("BPM_USER_FUSED", "1" if fused else "0")
    src, _k = NF.hip_source(variant, terms=(fused == "terms"))
    eng.set_device_likelihood(src, NF.box_params(r.d))
    is_fused, why = eng.device_likelihood_info()
    assert is_fused == (bool(fused) and r.d <= 512), why
    NF.assert_same_classes_and_close(eng.get_loglike(), r.ll0, 1e-12, 1e-12, "start ln-likes")
    eng.begin_run()
    g = 0
    prev = r.X0
    for k in (1, 4, 2, 2):
        eng.step(k)
        g += k
        st = _check_counters(eng, r, g - 1)
        now = eng.get_state()
        # the accept decisions of the k generations of this call: a chain the oracle accepted in one of them moved -- every chain that came back from
        # ll_cur = -inf among them -- and, where no outlier reset rewrites rows, nobody else did
        changed = np.any(now != prev, axis=1)
        accepted = np.any(r.acc[g - k:g], axis=0)
        back = np.any(r.from_minf[g - k:g], axis=0)
        assert np.all(changed[accepted]) and np.all(changed[back]), (g, np.nonzero(accepted & ~changed)[0])
        if "outlier_every" not in r.kw:
            assert np.array_equal(changed, accepted), (g, np.nonzero(changed != accepted)[0])
        prev = now
        np.testing.assert_allclose(now, r.X[g], rtol=1e-11, atol=1e-13)
        NF.assert_same_classes_and_close(eng.get_loglike(), r.ll[g], 1e-11, 1e-12, "ln-likes after generation %d" % (g - 1))
    assert g == NF.GENS and sum(int(np.count_nonzero(m)) for m in r.from_minf) >= 1
    assert st["n_outlier_resets"] == r.resets[-1]
    _check_end(eng, r, st, ll_history=True)
    eng.close()


def test_trace_ll_statistics_on_a_history_with_every_value_class():
    """param_est_trace's ll_min / ll_max / ll_mean (bpm_trace_bins) over an ln-like history that holds -inf, +inf and NaN beside finite values -- a sampler's
    own history, where tests/test_gpu_traces.py installs histories whose ln-likes come from the Gaussian target (NaN, never an infinity): NumPy's answer
    over get_loglike_history(), exact values and what is not finite exactly, the mean within the bound tests/test_traces_host.py derives."""
    from bipymc_amd import traces as TR
    from test_traces_host import check_against_numpy
    r = NF.oracle_box_run("dream-d8-N700-outlier", "bands")
    eng = _engine(algo=r.algo, n_chains=r.N, dim=r.d, target_id=R.TARGET_HOST, target_params=None, seed=r.seed, **r.kw)
    eng.set_state(r.X0)
    eng.set_device_likelihood(NF.hip_source("bands", terms=True)[0], NF.box_params(r.d))
    eng.begin_run()
    eng.step(NF.GENS)
    H, LL = eng.get_history(), eng.get_loglike_history()
    NF.assert_same_classes_and_close(LL, r.ll_history, 1e-11, 1e-12, "ln-like history")
    nan_, pinf, minf = NF.value_classes(LL)
    assert nan_.any() and pinf.any() and minf.any() and np.isfinite(LL).any()
    chains = list(dict.fromkeys([0, r.N - 1, int(np.argwhere(nan_)[0][1])]))
    for n_burn, every in ((0, 1), (r.N * 2 + 1, 3)):
        pt = TR.compute(eng.trace_bins, eng.trace_chains, TR.single_process_allgather, n_burn, eng.n_chains, eng.history_rows(), eng.dim,
                        every=every, chains=chains)
        check_against_numpy(pt, H, LL, n_burn, every, chains)
    eng.close()


# ------------------------------------------------------------------ 1. the box as a torch function on the device
_DEVICE = [(c[0], v) for c in NF.DEVICE_CASES for v in NF.VARIANTS]


@pytest.mark.parametrize("name,variant", _DEVICE, ids=["%s-%s" % t for t in _DEVICE])
def test_device_resident_likelihood_on_nonfinite_ln_likes(name, variant):
    """test_gpu_parity.py::test_device_resident_likelihood_against_oracle's loop (bpm_propose_device / bpm_commit_device) with the bounded-support function
    evaluated by torch on the device, at that test's three shapes; a child process that imports torch first, like there (tests/_torch_worker.py)."""
    import importlib.util
    if importlib.util.find_spec("torch") is None:
        pytest.skip("PyTorch is not installed")
    out = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(HERE, "_torch_worker.py"), "device_nonfinite", name, variant],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_LIMIT_S + 30)
    assert out.returncode == 0 and b"device_nonfinite ok" in out.stdout, out.stdout.decode()[-3000:]


# ------------------------------------------------------------------ 2. the shipped targets from overflow start rows, on the shipped path
@pytest.mark.parametrize("case", NF.OVERFLOW_CASES, ids=NF.OVERFLOW_IDS)
def test_shipped_targets_from_overflow_rows_equal_the_oracle(case):
    """Rows 1 and 5 of the start at magnitude 1e160 (z * z overflows; gamma (a - b) stays finite): the Gaussian and the mixture give ln-like NaN (the
    Gaussian at rho = 0: -inf), the banana -inf, and every chain that draws such a row as a partner proposes at that scale.  The shipped path -- own queue,
    no trace, the specialised instantiations, the planned front's scalar loads of ll_cur, the banana's lean form (ll_cur re-evaluated from the row, accepts
    counted per wavefront by ballot), synchronous DE-MC's x_next branch -- against the oracle over 8 generations, at the dispatch-table test's sizes:
    accept counts equal, n_nan_alpha equal AND positive, state / ln-like / two history rows as everywhere in tests/test_gpu_shipped_path.py with NaN,
    +inf and -inf each at the oracle's positions.

    DREAM runs with burnin_gen = 0 here, on purpose: from these starts the ORACLE'S OWN p_cr becomes NaN during CR adaptation (a jump distance of a
    proposal at 1e160 is inf, inf / inf after normalisation), so the reference defines nothing to compare with; adaptation on ln-likes that are not
    finite is covered by the box likelihood above, whose states stay finite."""
    algo, N, d, tid, params, seed, X0, kw, launches = NF.overflow_case(*case)
    _run_both(algo, N, d, tid, params, seed, X0, NF.OVERFLOW_GENS, kw, hist_rows=(2, NF.OVERFLOW_GENS), launches=launches, nonfinite=True)


# ------------------------------------------------------------------ 3. alternative kernel paths, bit for bit
def test_alternative_kernel_paths_from_overflow_rows():
    """tests/test_gpu_api.py::test_alternative_kernel_paths_on_one_gpu on starts with two overflow rows (tests/_nonfinite_worker.py: DREAM Gaussian d = 100
    N = 96, DREAM mixture d = 8 N = 101 with two pairs, DE-MC banana N = 77; 10 generations): the general instantiation (nohot), draws inside the kernel
    (noplan), one work item per local chain (mode1), the lean form at any size (lean; lean,mode1) and HIP stream launches must leave the default path's
    state, ln-likes, ln-like history, accept counts and NaN count, bit for bit (NaNs in equal positions); the NaN count is positive.  Every child runs
    under `timeout`; after one that did not exit with 0 no further child is started."""
    from bipymc_amd import _lib as L
    assert os.path.exists(L.TEST_LIB_PATH), "build_variants/libbipymc_test.so missing: make -C bipymc_amd/csrc"
    settings = [("", {}), ("nohot", {}), ("noplan", {}), ("mode1", {}), ("lean", {}), ("lean,mode1", {}), ("", {"BPM_DIRECT_QUEUE": "0"})]
    res = []
    with tempfile.TemporaryDirectory() as td:
        for i, (paths, extra) in enumerate(settings):
            env = dict(os.environ)
            for k in ("BPM_TEST_PATHS", "BPM_DIRECT_QUEUE", "BPM_QUEUE_INFLIGHT"):
                env.pop(k, None)
            if paths:                              # (read by the test variant of the library only)
                env["BPM_TEST_PATHS"] = paths
                env["BPM_LIB_PATH"] = L.TEST_LIB_PATH
            env.update(extra)
            f = os.path.join(td, "o%d.npz" % i)
            out = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(HERE, "_nonfinite_worker.py"), f], env=env,
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_LIMIT_S + 30)
            assert out.returncode == 0, (paths, extra, out.returncode, out.stdout.decode()[-3000:])      # (raises: nothing more is started)
            with np.load(f) as z:
                res.append({k: z[k] for k in z.files})
    ref = res[0]
    assert len(ref) == 12
    for name in ("dream_gauss100", "dream_mix8", "demc_banana"):
        assert ref[name + "_counts"][2] > 0 and ref[name + "_counts"][0] > 0, (name, ref[name + "_counts"])
        assert not np.all(np.isfinite(ref[name + "_ll_history"]))
    for (paths, extra), got in zip(settings[1:], res[1:]):
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (paths, extra, k)


# ------------------------------------------------------------------ 4. ranks
def _single_rank(case):
    from _push_worker import case_spec, start_state
    (tid, tp, d), algo, N, kw, G = case_spec(case)
    one = _engine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, **kw)
    one.set_state(start_state(case, N, d))
    one.begin_run(flip=0.4)
    one.step(G)
    st = one.stats()
    ref = dict(hist=one.get_history(), ll_hist=one.get_loglike_history(), state=one.get_state(), ll=one.get_loglike(), st=st)
    one.close()
    return ref


@pytest.mark.parametrize("exchange", ["push", "replay"])
def test_two_ranks_from_overflow_rows_equal_one_rank(exchange):
    """tests/_push_worker.py's case dream_gauss100_overflow (dream_gauss100 with one row of magnitude 1e160 in each rank's share) as a local group of
    R = 2 ranks: over the push exchange (owners store accepted rows into the peer's replica) and over the replay exchange (accept bytes travel, the
    receiving rank recomputes the accepted proposals -- a NaN alpha must be a 0 byte).  Every rank's replica, every chain's history and ln-like history
    equal the single-rank run bit for bit with NaNs in equal positions; the ranks' NaN counts and accept counts sum to the single rank's.  (The existing
    group drivers compare with np.array_equal without equal_nan, so the comparison is made here.)"""
    from bipymc_amd import _lib as L
    from _push_worker import case_spec, start_state
    case, R_ = "dream_gauss100_overflow", 2
    (tid, tp, d), algo, N, kw, G = case_spec(case)
    x0 = start_state(case, N, d)
    bad = np.nonzero(~np.isfinite(x0).all(axis=1) | (np.abs(x0).max(axis=1) > 1e100))[0]
    assert sorted(bad // (N // R_)) == [0, 1]                                   # one overflow row in each rank's share
    ref = _single_rank(case)
    assert ref["st"]["n_nan_alpha"] > 0 and np.isnan(ref["ll_hist"]).any()
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [_engine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, rank=r, world_size=R_, nccl_uid=uid, lib=L.load_test(), **kw)
             for r in range(R_)]
    arr = (C.c_void_p * R_)(*[e._h for e in ranks])
    if exchange == "push":
        blobs = [e.push_export() for e in ranks]
        for e in ranks:
            e.push_connect(blobs)
        ok = C.c_int32(0)
        L.check(ranks[0].lib.bpm_push_selftest(arr, R_, C.byref(ok)), ranks[0].lib)
        assert ok.value == 1
    for e in ranks:
        e.set_state(x0)
        e.begin_run(flip=0.4)
        if exchange == "replay":
            e.set_exchange(mode="replay")
    L.check(ranks[0].lib.bpm_local_group_step(arr, R_, G), ranks[0].lib)
    xs = ranks[0].exchange_stats()
    assert xs["mode"] == exchange
    if exchange == "push":
        assert xs["push_gens"] == G
    else:
        assert xs["replay_gens"] == G - kw["burnin_gen"]                       # (CR adaptation runs dense)
    n_local = N // R_
    H = np.concatenate([e.get_history() for e in ranks], axis=1)
    LLH = np.concatenate([e.get_loglike_history() for e in ranks], axis=1)
    assert np.array_equal(H, ref["hist"], equal_nan=True)
    assert np.array_equal(np.isnan(LLH), np.isnan(ref["ll_hist"])) and np.array_equal(LLH, ref["ll_hist"], equal_nan=True)
    sts = [e.stats() for e in ranks]
    for r, e in enumerate(ranks):
        assert np.array_equal(e.get_state(), ref["state"], equal_nan=True)     # every replica
        assert np.array_equal(e.get_loglike(), ref["ll"][r * n_local:(r + 1) * n_local], equal_nan=True)
        assert np.array_equal(sts[r]["p_cr"], ref["st"]["p_cr"], equal_nan=True)
        assert np.array_equal(sts[r]["n_cr_updates"], ref["st"]["n_cr_updates"])
        assert sts[r]["n_nan_alpha"] > 0                                        # (each rank owns one of the two rows)
    assert sum(s["n_nan_alpha"] for s in sts) == ref["st"]["n_nan_alpha"]
    assert sum(s["local_n_accepted"] for s in sts) == ref["st"]["local_n_accepted"] > 0
    for e in ranks:
        e.close()
