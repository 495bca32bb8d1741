"""The drop-in surface on the GPU: the reference's own test scenarios (tests/test_dblgauss.py,
tests/test_banana.py, tests/test_100dgauss.py) driven through bipymc_amd.DeMcMpi / DreamMpi, the
host-callback ln_like_fn path, checkpoints, and size-independent properties at BASELINE sizes."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_cfg1_dream_bimodal_reference_scenario(golden_dir):
    """BASELINE config 1 / tests/test_dblgauss.py:135-140,43-69: DREAM n_chains=10, n=100000, n_burn=40000."""
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import dblgauss_rv
    np.random.seed(42)
    target = dblgauss_rv.BimodeGauss_2D()
    s = DreamMpi(target.ln_like, np.zeros(2), n_chains=10, mpi_comm=None, n_cr_gen=50, burnin_gen=2000)
    assert s.uses_device_target
    s.run_mcmc(100000)
    theta_est, sig_est, chain = s.param_est(n_burn=40000)
    theta_full, _, full_chain = s.param_est(n_burn=0)
    assert full_chain.shape == (100000, 2) and chain.shape == (60000, 2)
    # the reference's assertion (test_dblgauss.py:67-69)
    assert abs(theta_est[0] - 1.5) <= 0.1 and abs(theta_est[1] - 1.5) <= 0.1
    # exact per-axis std is sqrt(0.8125) = 0.9014; 10 chains, 6000 generations: 5 %
    assert abs(sig_est[0] - 0.9014) < 0.05 and abs(sig_est[1] - 0.9014) < 0.05
    assert 0.05 < s.acceptance_fraction < 0.6
    # statistical anchor recorded from the genuine reference (same config, shorter run): same regime
    ref = json.load(open(os.path.join(golden_dir, "e2e_anchor_cfg1.json")))
    assert abs(s.acceptance_fraction - ref["acceptance_fraction"]) < 0.08
    assert s.p_cr.shape == (3,) and abs(s.p_cr.sum() - 1.0) < 1e-12
    # p_cr against the reference's own runs (tests/golden/e2e_anchor_cfg1_seeds.json: the same configuration under six
    # np.random seeds, recorded by oracle/gen_golden.py).  ONE reference run is a noisy estimate -- seed 42 ends at
    # (0.18, 0.38, 0.44), the five others at 0.30-0.34 / 0.32-0.35 / 0.32-0.37 -- so the anchor is the family's median,
    # (0.312, 0.334, 0.365).  Tolerance 0.08 per component: the family's own standard deviation is 0.05 / 0.02 / 0.04, the
    # seed-to-seed standard deviation of this build's sampler (12 seeds on the CPU oracle) 0.018 / 0.014 / 0.017.
    fam = json.load(open(os.path.join(golden_dir, "e2e_anchor_cfg1_seeds.json")))
    assert np.max(np.abs(s.p_cr - np.array(fam["p_cr_median"]))) < 0.08, (s.p_cr, fam["p_cr_median"])
    assert abs(s.acceptance_fraction - fam["acceptance_median"]) < 0.08
    assert s.n_accepted + s.n_rejected == 9999 * 10 + 1


def test_demc_bimodal_and_banana_reference_scenarios():
    """tests/test_dblgauss.py:130-133 (DE-MC n_chains=20) and tests/test_banana.py:43-72,118-121."""
    from bipymc_amd import DeMcMpi
    from bipymc_amd.utils import banana_rv, dblgauss_rv
    np.random.seed(42)
    s = DeMcMpi(dblgauss_rv.BimodeGauss_2D().ln_like, np.zeros(2), n_chains=20)
    s.run_mcmc(100000)
    theta_est, _, _ = s.param_est(n_burn=40000)
    assert abs(theta_est[0] - 1.5) <= 0.1 and abs(theta_est[1] - 1.5) <= 0.1
    banana = banana_rv.Banana_2D(sigma1=1, sigma2=1)
    s = DeMcMpi(banana.ln_like, np.array([0.0, 0.0]), n_chains=20)
    s.run_mcmc(100000)
    _, _, chain = s.param_est(n_burn=20000)
    y1, y2 = chain[:, 0], chain[:, 1]
    # fraction of samples above the pdf levels 0.18 / 0.018; analytic values 0.5070 / 0.9507
    f1 = np.count_nonzero(banana.check_prob_lvl(y1, y2, 0.18)) / y1.size
    f2 = np.count_nonzero(banana.check_prob_lvl(y1, y2, 0.018)) / y1.size
    assert abs(f1 - 0.5070) <= 0.05 and abs(f2 - 0.9507) <= 0.05      # reference tolerance (test_banana.py:71-72)


def test_100d_gauss_reference_scenario():
    """tests/test_100dgauss.py:100-110: DE-MC n_chains=200 and DREAM n_chains=100, n=500000, n_burn=200000."""
    from bipymc_amd import DeMcMpi, DreamMpi
    from bipymc_amd.utils import d100_gauss
    np.random.seed(42)
    gauss = d100_gauss.Gauss_100D()
    for mk in (lambda: DeMcMpi(gauss.ln_like, np.zeros(100), n_chains=200),
               lambda: DreamMpi(gauss.ln_like, np.zeros(100), n_chains=100, n_cr_gen=50, burnin_gen=2000)):
        s = mk()
        s.run_mcmc(500000)
        theta_est, sig_est, chain = s.param_est(n_burn=200000)
        assert abs(theta_est[0]) <= 0.2 and abs(theta_est[1]) <= 0.2            # test_100dgauss.py:67-69
        assert chain.shape[0] == 300000


def test_product_and_test_variant_run_side_by_side_in_one_process():
    """Round 5 regression: the product library and the test variant in ONE process, both samplers on their own AQL queues, alternating.  The queue
    locates kernels by name; with equal names the library loaded second dispatched the first one's kernels -- a memory fault as soon as the two
    argument blocks differed (the product's has no trace fields).  Same configuration, same seed: bit-identical states, and the test variant's
    traced run (HIP stream, general kernel with the trace code) agrees as well."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, d = d100_gauss.Gauss_100D(rho=0.5, dim=100)._bpm_target_spec()
    X0 = np.random.RandomState(3).normal(size=(512, d)) * np.sqrt(np.arange(d) + 1.0)
    kw = dict(algo=L.ALGO_DREAM, n_chains=512, dim=d, target_id=tid, target_params=tp, seed=19, burnin_gen=6, n_cr_gen=2)
    a = HipEngine(**kw)
    b = HipEngine(lib=L.load_test(), **kw)
    c = HipEngine(lib=L.load_test(), **kw)
    for e in (a, b, c):
        e.set_state(X0)
    c.set_trace(True)
    for e in (a, b, c):
        e.begin_run()
    for _ in range(4):                    # interleaved: both libraries' queues are live at the same time
        a.step(5); b.step(5); c.step(5)
    la, lb = a.launch_stats(), b.launch_stats()
    assert la["has_queue"] and lb["has_queue"] and la["direct"] >= 40 and lb["direct"] >= 40
    Xa, Xb, Xc = a.get_state(), b.get_state(), c.get_state()
    assert np.array_equal(Xa, Xb) and np.array_equal(Xa, Xc)
    assert np.array_equal(a.get_history(), b.get_history())
    assert a.stats()["local_n_accepted"] == b.stats()["local_n_accepted"] == c.stats()["local_n_accepted"]
    np.testing.assert_array_equal(a.stats()["p_cr"], b.stats()["p_cr"])
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("scenario", ["gauss100_dream", "gauss100_demc", "banana_dream", "banana_demc", "bimodal_demc"])
def test_reference_families_hold_the_device(scenario):
    """the reference's own scenarios through the drop-in classes ON THE DEVICE, held against the families the genuine
    reference produced (tests/golden/e2e_anchor_*.json, oracle/gen_anchor_families.py): DreamMpi N = 100 / DeMcMpi N = 200 on the 100-D Gaussian
    (tests/test_100dgauss.py:100-110: acceptance 0.2094 +- 0.0004, p_cr (0.177, 0.334, 0.491) +- 0.005 for DREAM; the population's variance grows
    from 1e-6 along the same curve), DreamMpi N = 10 / DeMcMpi N = 20 on the banana with the level fractions within 0.05 (tests/test_banana.py:60-72,
    118-127), DeMcMpi N = 20 on the bimodal target (tests/test_dblgauss.py:130-133).  Two seeds each; tolerances: tests/_anchors.py."""
    import _anchors as A
    from bipymc_amd import DeMcMpi, DreamMpi
    from bipymc_amd.utils import banana_rv, d100_gauss, dblgauss_rv
    doc = A.load(scenario)
    tgt = {"gauss100": d100_gauss.Gauss_100D(), "banana": banana_rv.Banana_2D(sigma1=1.0, sigma2=1.0), "bimodal": dblgauss_rv.BimodeGauss_2D()}[doc["target"]]
    d = 100 if doc["target"] == "gauss100" else 2
    N = doc["n_chains"]
    for seed in (42, 7):
        cls = DreamMpi if doc["algo"] == "dream" else DeMcMpi
        s = cls(tgt.ln_like, np.zeros(d), n_chains=N, seed=seed, **doc["kwargs"])
        assert s.uses_device_target
        s.run_mcmc(doc["n"])
        _, _, full = s.param_est(n_burn=0)
        T = full.shape[0] // N
        got = A.summarize(doc, full.reshape(T, N, d), s.acceptance_fraction, s.p_cr if doc["algo"] == "dream" else None)
        s._engine.close()
        A.check(scenario, got, "device, seed %d" % seed)


def test_headline_configuration_at_the_references_own_p_cr(golden_dir):
    """The genuine reference AT THE HEADLINE SIZE (oracle/gen_anchor_cfg2.py -> tests/golden/e2e_anchor_cfg2_headline.json: DreamMpi, 100-D Gaussian, 8192
    chains from exact draws of the target, n_cr_gen = 50, burnin_gen = 200; two seeds, ~45 minutes each): with p_cr uniform (generations 1-50) it accepts
    0.165 of its updates; its CR adaptation then collapses to a one-hot p_cr within one generation (the zero-variance clamp of dream.py:129 meets the
    per-update re-estimation of dream.py:134-140; see tests/test_oracle_golden.py::test_headline_configuration_at_fixed_p_cr...) and the acceptance becomes
    that of the surviving CR value.  The device at the reference's own p_cr -- uniform, and the one-hot vector each reference run ended with, installed
    through bpm_set_adapt_state -- must accept the same fraction at the same size (tolerance 0.006); what differs between the two is the adaptation's
    outcome (this build: (0.25, 0.27, 0.48), a documented deviation), not the update."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    doc = json.load(open(os.path.join(golden_dir, "e2e_anchor_cfg2_headline.json")))
    g = d100_gauss.Gauss_100D()
    tid, tp, d = g._bpm_target_spec()
    N = 8192

    def acceptance(p_cr, seed, gens=50):
        np.random.seed(seed)
        e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=seed, burnin_gen=0, n_cr_gen=50)
        e.set_state(g.rvs(N))
        e.set_adapt_state(p_cr=p_cr, delta_m=np.zeros(3), n_cr_updates=np.zeros(3))
        e.begin_run()
        e.step(gens)
        st = e.stats()
        e.close()
        return st["local_n_accepted"] / float(st["local_n_accepted"] + st["local_n_rejected"])
    uniform_ref = np.mean([np.mean([s_["window_acceptance"] for s_ in r["trajectory"] if s_["generation"] <= 50]) for r in doc["runs"]])
    assert abs(acceptance([1 / 3.0] * 3, 11) - uniform_ref) < 0.006, uniform_ref
    for k, r in enumerate(doc["runs"]):
        p = np.array(r["p_cr_final"])
        assert np.max(p) > 1.0 - 1e-12 and np.sum(p > 1e-12) == 1          # the reference's own p_cr at this configuration: one-hot
        onehot = (p > 0.5).astype(float)
        assert abs(acceptance(onehot, 12 + k) - r["acceptance_after_burnin"]) < 0.006, (p, r["acceptance_after_burnin"])


def test_host_callback_equals_device_target():
    """An arbitrary Python ln_like_fn (samplers.py:36-43) takes the propose/commit path; with the same
    target it must reproduce the fused device path (same draws, ln_like equal to rounding)."""
    from bipymc_amd import DeMcMpi, DreamMpi
    from bipymc_amd.utils import banana_rv, d100_gauss
    g = d100_gauss.Gauss_100D(rho=0.5, dim=10)
    calls = []

    def py_ll(theta, offset=0.0):
        assert isinstance(theta, np.ndarray) and theta.shape == (10,) and theta.dtype == np.float64
        calls.append(1)
        return float(g.ln_like(theta)) + offset

    a = DreamMpi(g.ln_like, np.ones(10), n_chains=16, n_cr_gen=3, burnin_gen=10, seed=5)
    b = DreamMpi(py_ll, np.ones(10), n_chains=16, n_cr_gen=3, burnin_gen=10, seed=5, ln_kwargs={"offset": 0.0})
    assert a.uses_device_target and not b.uses_device_target
    a.run_mcmc(16 * 31)
    b.run_mcmc(16 * 31)
    assert len(calls) == 16 + 16 * 30                       # once per chain at init, once per chain update
    np.testing.assert_allclose(b.param_est(0)[2], a.param_est(0)[2], rtol=1e-9, atol=1e-12)
    assert b.n_accepted == a.n_accepted
    np.testing.assert_allclose(b.p_cr, a.p_cr, rtol=1e-9)
    # DE-MC with snooker and an odd dimension through the host path
    t3 = lambda th: -0.5 * float(np.sum(th ** 2))
    c = DeMcMpi(t3, np.zeros(3), n_chains=12, seed=9, p_snooker=0.2)
    c.run_mcmc(12 * 2001)
    m, sd, _ = c.param_est(12 * 500)
    assert np.all(np.abs(m) < 0.15) and np.all(np.abs(sd - 1.0) < 0.15)
    # priors returning -inf (examples/ex_para_fit.py:45-55): proposals outside the support are rejected
    def bounded(th):
        return -np.inf if np.any(np.abs(th) > 1.0) else 0.0
    d = DeMcMpi(bounded, np.zeros(2), varepsilon=1e-2, n_chains=16, seed=3)
    d.run_mcmc(16 * 801)
    ch = d.param_est(16 * 200)[2]
    assert np.all(np.abs(ch) <= 1.0) and abs(ch.std() - 1 / np.sqrt(3)) < 0.05


def test_callback_transports_agree():
    """One likelihood, five ways to call it (samplers.py:36-43 calls ln_like_fn row by row): per row, vectorised in one piece, vectorised with the
    read-back in overlapped pieces, the pieces evaluated by a pool of host threads, and as a torch function on the device (vectorized="device").
    Body: tests/_torch_worker.py::transports, in a child process that imports torch first (one HIP runtime per process)."""
    import importlib.util
    if importlib.util.find_spec("torch") is None:      # (NOT imported here: torch brings HIP / HSA / RCCL copies of its own, and importing it into a process
        pytest.skip("PyTorch is not installed")       #  whose library is already loaded breaks RCCL's first contact for every later test)
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "_torch_worker.py"), "transports"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0 and b"transports ok" in r.stdout, r.stdout.decode()[-3000:]


def test_hip_source_likelihood_through_the_sampler_classes(tmp_path):
    """ln_like_fn = HipLikelihood(source, params) (bipymc_amd/device_likelihood.py): DreamMpi / DeMcMpi run it inside the generation loop.  The same seed
    with the same formula as a vectorised NumPy callback (the host-callback transport) gives the same run -- accept counts equal, chains to 1e-9 -- and the
    posterior of a 6-D Gaussian with unequal scales comes out; a checkpoint + warm start goes on with the device likelihood; a prior's -inf is honoured."""
    from bipymc_amd import DeMcMpi, DreamMpi, HipLikelihood
    d = 6
    mu, sig = np.arange(d) * 0.5, 1.0 + 0.5 * np.arange(d)
    src = """
    __device__ double ln_like(const double* x, int d, const double* p) {
        if (x[0] < p[2 * d]) return -INFINITY;                       // a prior: x_0 above a bound
        double s = 0.0;
        for (int j = 0; j < d; ++j) { const double z = (x[j] - p[j]) / p[d + j]; s += z * z; }
        return -0.5 * s;
    }"""
    bound = -1.0

    def np_ll(X):
        X = np.atleast_2d(X)
        z = (X - mu) / sig
        s = np.zeros(len(X))
        for j in range(d):                                            # (the kernel's summation order)
            s += z[:, j] * z[:, j]
        return np.where(X[:, 0] < bound, -np.inf, -0.5 * s)

    ll = HipLikelihood(src, params=np.concatenate([mu, sig, [bound]]), python_fn=lambda th: float(np_ll(th)[0]))
    assert ll.check()
    for cls, kw in ((DreamMpi, dict(n_cr_gen=10, burnin_gen=100)), (DeMcMpi, dict(p_snooker=0.1))):
        a = cls(ll, mu, varepsilon=1e-3, n_chains=512, seed=21, **kw)
        b = cls(np_ll, mu, varepsilon=1e-3, n_chains=512, seed=21, vectorized=True, **kw)
        assert a._hip_likelihood is ll and not a.uses_device_target and b._hip_likelihood is None
        assert a._engine.device_likelihood_info()[0], a._engine.device_likelihood_info()[1]      # the update kernel itself was compiled around the likelihood
        a.run_mcmc(512 * 301)
        b.run_mcmc(512 * 301)
        assert a.local_n_accepted == b.local_n_accepted and a.local_n_rejected == b.local_n_rejected
        np.testing.assert_allclose(a.param_est(0)[2], b.param_est(0)[2], rtol=1e-9, atol=1e-11)
        ch = a.param_est(512 * 150)[2]
        assert ch[:, 0].min() >= bound
        # x_0 ~ N(0, 1) truncated at -1: mean 0.2876, the others untruncated
        assert abs(ch[:, 0].mean() - 0.2876) < 0.05
        np.testing.assert_allclose(ch[:, 1:].mean(axis=0), mu[1:], atol=0.12 * sig[1:].max())
        np.testing.assert_allclose(ch[:, 1:].std(axis=0), sig[1:], rtol=0.08)
    f = str(tmp_path / "ck.npz")
    a = DreamMpi(ll, mu, varepsilon=1e-3, n_chains=64, seed=3, n_cr_gen=5, burnin_gen=20, h5_file=f)
    a.run_mcmc(64 * 30)
    a.save_state(f)
    a2 = DreamMpi(ll, None, dim=d, n_chains=64, seed=3, n_cr_gen=5, burnin_gen=20, h5_file=f, warm_start=True)
    np.testing.assert_allclose(a2._engine.get_loglike(), a._engine.get_loglike(), rtol=0, atol=0)
    a2.run_mcmc(64 * 10)
    assert a2.param_est(0)[2].shape == (64 * 39, d)            # (demc.py:79: 29 + 9 generations behind the start row)
    with pytest.raises(Exception, match="does not compile"):
        DreamMpi(HipLikelihood("double ln_like(x) { }"), mu, n_chains=8, seed=1)
    # the serial-API sampler (samplers.py:237-336, delayed-accept form) takes it too: the same run as with the formula as a Python callable
    from bipymc_amd.samplers import DeMc
    runs = []
    for fn in (ll, lambda th: float(np_ll(th)[0])):
        sd = DeMc(fn, n_chains=32, seed=9)
        sd.run_mcmc(32 * 40, mu, varepsilon=1e-2)
        runs.append((sd.n_accepted, sd.param_est(0)[2]))
    assert runs[0][0] == runs[1][0]
    np.testing.assert_allclose(runs[0][1], runs[1][1], rtol=1e-9, atol=1e-11)


def test_hip_source_likelihood_on_every_launch_path():
    """The update kernel compiled around a HIP-source likelihood is dispatched through the library's own queue (found by its lowered name) -- or, without the
    queue (BPM_DIRECT_QUEUE=0) or on request (BPM_USER_FUSED=2), launched on the HIP stream; BPM_USER_FUSED=0 runs the likelihood as a kernel of its own between
    the proposal and the commit kernel.  Same draws, same arithmetic in the same order: state, ln-likes, CR statistics and accept counts after a burn-in and a
    steady stretch are equal bit for bit on all four paths (DREAM d = 100 and d = 8, DE-MC d = 2 with snooker)."""
    import subprocess
    import tempfile
    code = r'''
import os, sys, numpy as np
sys.path.insert(0, os.getcwd())
from bipymc_amd import _lib as L
from bipymc_amd.engine import HipEngine
SRC = """__device__ double ln_like(const double* x, int d, const double* p) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) { const double z = (x[j] - p[j]) * p[d + j]; s += z * z; }
    return -0.5 * s;
}"""
out = []
for algo, d, N, kw in ((L.ALGO_DREAM, 100, 2048, dict(burnin_gen=8, n_cr_gen=2)), (L.ALGO_DREAM, 8, 5000, dict(burnin_gen=8, n_cr_gen=2)),
                       (L.ALGO_DEMC, 2, 3001, dict(p_snooker=0.2))):
    e = HipEngine(algo=algo, n_chains=N, dim=d, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=11, **kw)
    e.set_state(np.random.RandomState(d).normal(size=(N, d)))
    e.set_device_likelihood(SRC, np.concatenate([np.linspace(-1, 1, d), 1.0 / (1.0 + np.arange(d) % 3)]))
    fused, why = e.device_likelihood_info()
    assert fused == (os.environ.get("BPM_USER_FUSED", "1") != "0"), why
    e.begin_run(); e.step(5); e.step(1); e.step(14)
    st = e.stats()
    out += [e.get_state(), e.get_loglike(), np.asarray(st["p_cr"], dtype=float), np.array([st["local_n_accepted"], st["local_n_rejected"]], dtype=float)]
    ls = e.launch_stats()
    want_direct = fused and os.environ.get("BPM_DIRECT_QUEUE", "1") != "0" and os.environ.get("BPM_USER_FUSED", "1") == "1"
    assert (ls["direct"] > 0) == want_direct, ls
    e.close()
np.save(sys.argv[1], np.concatenate([o.reshape(-1) for o in out]))
'''
    res = []
    for extra in ({}, {"BPM_DIRECT_QUEUE": "0"}, {"BPM_USER_FUSED": "2"}, {"BPM_USER_FUSED": "0"}):
        env = dict(os.environ)
        for k in ("BPM_DIRECT_QUEUE", "BPM_USER_FUSED", "BPM_TEST_PATHS", "BPM_LIB_PATH"):
            env.pop(k, None)
        env.update(extra)
        with tempfile.TemporaryDirectory() as td:
            f = os.path.join(td, "o.npy")
            subprocess.check_call([sys.executable, "-c", code, f], env=env, cwd=os.path.join(os.path.dirname(__file__), ".."))
            res.append(np.load(f))
    for r in res[1:]:
        assert np.array_equal(res[0], r)


def test_hip_source_likelihood_replaced_by_another(monkeypatch):
    """bpm_set_device_likelihood on a sampler that already has one: the new likelihood -- its kernel, its parameter block and the update kernel compiled
    around it -- takes the old one's place whole (the queue forgets the old kernels' names and finds the new ones), and an install that fails leaves the
    installed one as it was.  Two engines built alike, one with the update kernel compiled around each likelihood, one with BPM_USER_FUSED=0 (the variable is
    read at every install), go through A -> 6 generations -> B -> 6 generations (the rest of the burn-in and two steady ones: B's burn-in, steady and
    general instantiations all run) -> a source that does not compile -> 2 generations: state, ln-likes, CR statistics and accept counts equal bit for bit."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    N, d = 256, 8
    src_a = """__device__ double ln_like(const double* x, int d, const double* p) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) { const double z = (x[j] - p[j]) * p[d + j]; s += z * z; }
    return -0.5 * s;
}"""
    src_b = src_a.replace("-0.5 * s", "-0.5 * (2.0 * s)")
    assert src_b != src_a
    par_a = np.concatenate([np.linspace(-1, 1, d), 1.0 / (1.0 + np.arange(d) % 3)])
    par_b = np.concatenate([np.linspace(0.5, -0.5, d), 1.0 / (2.0 + np.arange(d) % 2)])
    broken = "__device__ double ln_like(const double* x, int d, const double* p) { return x[0] }"
    X0 = np.random.RandomState(5).normal(size=(N, d))

    def run(fused):
        if fused:
            monkeypatch.delenv("BPM_USER_FUSED", raising=False)
        else:
            monkeypatch.setenv("BPM_USER_FUSED", "0")
        e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=L.TARGET_HOST_CALLBACK, target_params=None, seed=11, burnin_gen=10, n_cr_gen=2)
        e.set_state(X0)
        e.set_device_likelihood(src_a, par_a)
        assert e.device_likelihood_info()[0] == fused, e.device_likelihood_info()[1]
        e.begin_run()
        d0 = e.launch_stats()["direct"]
        e.step(6)
        d1 = e.launch_stats()["direct"]
        e.set_device_likelihood(src_b, par_b)
        assert e.device_likelihood_info()[0] == fused, e.device_likelihood_info()[1]
        e.step(6)
        d2 = e.launch_stats()["direct"]
        if fused and d1 > d0:
            assert d2 > d1, (d0, d1, d2)      # the new kernels were found by their names after the old ones were forgotten
        with pytest.raises(L.BpmError, match="does not compile"):
            e.set_device_likelihood(broken, par_b)
        assert e.device_likelihood_info()[0] == fused, e.device_likelihood_info()[1]
        e.step(2)
        st = e.stats()
        return e, [e.get_state(), e.get_loglike(), np.asarray(st["p_cr"], dtype=float), np.array([st["local_n_accepted"], st["local_n_rejected"]])]

    e1, r1 = run(True)
    e2, r2 = run(False)
    for a, b in zip(r1, r2):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(r1[1]))
    e1.close()      # (raises if bpm_destroy reports an error)
    e2.close()


def test_bench_runs_without_torch_and_without_burn_in_for_the_kernel_trace():
    """tools/profile_bench.sh traces `python bench.py ... --no-torch --burnin-gens 0`: under rocprofv3 a process that loaded torch's HIP runtime, or has run the
    burn-in kernels, shows a mode of slow steady-state launches that un-profiled runs do not have (profiles/r05_rocprof_torch_artefact.txt).  The flags must
    keep producing the contract's one JSON line -- same metric, same workload, roofline from the live time stamps -- with torch never imported."""
    import json
    import subprocess
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "40", "--warmup", "5", "--no-cpu-baseline", "--no-other-configs", "--no-moments",
                        "--preheat", "0", "--no-torch", "--burnin-gens", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert line["metric"] == "chain-updates/sec" and line["n_gpus"] == 1 and line["steps"] == 40 and line["value"] > 1e8
    assert line["config"]["torch_in_the_process"] is False and line["config"]["burnin_generations"] == 0
    assert line["roofline"]["bound"] == "hbm" and 0.3 < line["roofline"]["frac"] < 1.0 and line["roofline"]["measured_copy_GBps"] is None
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--no-torch"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=root)
    assert r2.returncode != 0                    # (the ranks of a world meet through torch.distributed: refused, on every rank)


def test_plain_bench_run_is_the_headline_and_dumps_what_the_timed_generations_computed(tmp_path):
    """`bench.py --steps K --warmup W` without --full measures the headline and nothing beside it; --dump-outputs writes the state the K timed
    generations ended in (the state whose hash the line carries), its ln-likes and the history rows the last of them appended."""
    import hashlib
    import subprocess
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5", "--dump-outputs", out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert line["metric"] == "chain-updates/sec" and line["steps"] == 30 and line["value"] > 1e8 and line["dtype"] == "f64"
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / 8192 - 1.0) < 1e-9
    assert "configs" not in line and "cpu_baseline" not in line and line["posterior"]["evaluated"] is False
    assert line["roofline"]["measured_copy_GBps"] is None and line["roofline"]["avg_launch_us_event_pairs"] is None
    X, ll = np.load(os.path.join(out, "state.npy")), np.load(os.path.join(out, "ln_like.npy"))
    assert X.shape == (8192, 100) and X.dtype == np.float64 and np.all(np.isfinite(X)) and ll.shape == (8192,)
    assert hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest()[:16] == line["config"]["final_state_sha256_16"]
    assert np.array_equal(np.load(os.path.join(out, "history_last_step.npy")), X)
    np.testing.assert_allclose(np.load(os.path.join(out, "ln_like_history_last_step.npy")), ll, rtol=1e-12, atol=0)


def test_nan_ratio_raises_like_numpy():
    """both ln_like values -inf -> alpha NaN -> the reference's np.random.choice raises ValueError (samplers.py:336)"""
    from bipymc_amd import DeMcMpi
    s = DeMcMpi(lambda th: -np.inf, np.zeros(2), n_chains=8, seed=1)
    with pytest.raises(ValueError):
        s.run_mcmc(8 * 3)


def test_nan_ratio_raises_on_the_device_paths_too():
    """The same start -- every chain outside the support, so both ln-likes are -inf and alpha is NaN -- on the shipped banana target (the fused kernels,
    lean form: a start at 1e160 overflows to -inf) and on a HipLikelihood of a box (tests/_nonfinite_cases.py; the run-time compiled update kernel)."""
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import _nonfinite_cases as NF
    from bipymc_amd import DeMcMpi, HipLikelihood
    from bipymc_amd.utils import banana_rv
    s = DeMcMpi(banana_rv.Banana_2D().ln_like, np.full(2, 1e160), n_chains=8, seed=1)
    assert s.uses_device_target
    with pytest.raises(ValueError):
        s.run_mcmc(8 * 3)
    d = 3
    box = HipLikelihood(NF.hip_source("box", terms=False)[0], params=NF.box_params(d), python_fn=NF.BoxLikelihood(d, "box"))
    s = DeMcMpi(box, 10.0 * NF.sigma_of(d), n_chains=8, seed=1)
    assert not s.uses_device_target
    with pytest.raises(ValueError):
        s.run_mcmc(8 * 3)


@pytest.mark.parametrize("ext", [".npz", ".h5"])
def test_checkpoint_warm_start_gpu(tmp_path, ext):
    """demc.py:198-233 through the device engine: the NumPy twin of the layout, and the reference's own HDF5 layout (h5py, or the
    HDF5 C library through ctypes)."""
    from bipymc_amd import DreamMpi, checkpoint
    from bipymc_amd.utils import dblgauss_rv
    if ext == ".h5" and checkpoint.hdf5_backend() is None:
        pytest.skip("neither h5py nor libhdf5 can be loaded on this machine")
    t = dblgauss_rv.BimodeGauss_2D()
    f = str(tmp_path / ("ck" + ext))
    s = DreamMpi(t.ln_like, np.zeros(2), n_chains=8, n_cr_gen=3, burnin_gen=10, seed=5, h5_file=f, checkpoint=4)
    s.run_mcmc(8 * 13)
    full = s.param_est(0)[2]
    s2 = DreamMpi(t.ln_like, None, n_chains=8, dim=2, n_cr_gen=3, burnin_gen=10, seed=5, h5_file=f, warm_start=True)
    assert np.array_equal(s2.param_est(0)[2], full)
    np.testing.assert_allclose(s2.p_cr, s.p_cr)
    s2.run_mcmc(8 * 6)                     # adaptation resumes: Welford moments rebuilt from the loaded rows
    assert s2.param_est(0)[2].shape == (8 * 18, 2)
    assert np.array_equal(s2.param_est(0)[2][:8 * 13], full)


def test_device_moments_equal_host_param_est():
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    g = d100_gauss.Gauss_100D(rho=0.5, dim=7)
    s = DreamMpi(g.ln_like, np.zeros(7), n_chains=24, seed=2, burnin_gen=20, n_cr_gen=5)
    s.run_mcmc(24 * 60)
    for n_burn in (0, 24 * 10, 24 * 10 + 5, 24 * 59 + 23):
        mean, std, chain = s.param_est(n_burn)
        cnt, s1, s2, sh = s._engine.reduce_moments(n_burn)
        assert cnt == chain.shape[0]
        np.testing.assert_allclose(sh + s1 / cnt, mean, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(np.sqrt(s2 / cnt - (s1 / cnt) ** 2), std, rtol=1e-9)


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3", "cfg5_local"])
def test_full_size_properties(cfg):
    """BASELINE full sizes, checked through size-independent properties: determinism (same seed ->
    same bits), history/state consistency, accept bookkeeping, finite log-likes, and movement."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import banana_rv, d100_gauss, mixture_nd
    if cfg == "cfg2":
        tid, tp, d = d100_gauss.Gauss_100D()._bpm_target_spec()
        kw = dict(algo=L.ALGO_DREAM, n_chains=8192, dim=d, burnin_gen=10, n_cr_gen=3)
        x0 = np.random.RandomState(0).normal(size=(8192, d)) * np.sqrt(np.arange(d) + 1.0)
        gens = 20
    elif cfg == "cfg3":
        tid, tp, d = banana_rv.Banana_2D()._bpm_target_spec()
        kw = dict(algo=L.ALGO_DEMC, n_chains=65536, dim=d, p_snooker=0.1)
        x0 = np.random.RandomState(0).normal(size=(65536, d)) + np.array([0, 1.0])
        gens = 30
    else:
        tid, tp, d = mixture_nd.BimodeGauss_ND(8)._bpm_target_spec()
        kw = dict(algo=L.ALGO_DREAM, n_chains=32768, dim=d, burnin_gen=10, n_cr_gen=3)
        rs = np.random.RandomState(0)
        x0 = np.where(rs.uniform(size=(32768, 1)) < 0.25, 0.0, 2.0) + 0.25 * rs.normal(size=(32768, d))
        gens = 30
    outs = []
    for rep in range(2):
        e = HipEngine(target_id=tid, target_params=tp, seed=77, **kw)
        e.set_state(x0)
        e.begin_run()
        e.step(gens)
        st = e.stats()
        H = e.get_history(gens - 1, gens + 1)
        X = e.get_state()
        assert np.array_equal(H[-1], X)                                     # last history row = current state
        moved = np.any(H[-1] != H[-2], axis=1)
        assert st["local_n_accepted"] + st["local_n_rejected"] == gens * kw["n_chains"] + 1
        assert 0.02 < st["local_n_accepted"] / (gens * kw["n_chains"]) < 0.9
        assert 0 < moved.sum() < kw["n_chains"]
        ll = e.get_loglike()
        assert np.all(np.isfinite(ll))
        np.testing.assert_allclose(ll, e.eval_loglike(X), rtol=1e-12, atol=1e-9)   # cache == fresh evaluation
        outs.append((X, st["local_n_accepted"], st["p_cr"]))
        e.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]     # bitwise reproducible
    assert np.array_equal(outs[0][2], outs[1][2])


def _prefetch_with_progress(path, capsys):
    """Read a large shared library into the page cache in 32 MiB chunks, one visible dot per chunk.  On a fresh box
    dlopen of the 573 MB librccl pages in from a cold image for minutes; done silently inside a captured test that
    looks like a hang to a watchdog that wants output every few minutes."""
    if not os.path.exists(path):
        return
    with capsys.disabled():
        sys.stdout.write("[paging in %s " % os.path.basename(path))
        sys.stdout.flush()
        with open(path, "rb", buffering=0) as f:
            while f.read(32 << 20):
                sys.stdout.write(".")
                sys.stdout.flush()
        sys.stdout.write("]")
        sys.stdout.flush()


def test_rccl_one_rank_communicator(capsys):
    """RCCL is loaded on demand; a one-rank communicator runs the in-place all-gather after each half
    generation on the sampler's stream and must not change any result."""
    _prefetch_with_progress("/opt/rocm/lib/librccl.so.1", capsys)
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, d = d100_gauss.Gauss_100D(dim=20)._bpm_target_spec()
    x0 = np.random.RandomState(0).normal(size=(64, d))
    res = []
    for uid in (None, HipEngine.unique_id()):
        e = HipEngine(algo=L.ALGO_DREAM, n_chains=64, dim=d, target_id=tid, target_params=tp, seed=3, nccl_uid=uid,
                      burnin_gen=5, n_cr_gen=2)
        e.set_state(x0)
        e.begin_run()
        e.step(12)
        res.append((e.get_state(), e.stats()["p_cr"]))
        e.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def _test_lib_path():
    from bipymc_amd import _lib as L
    assert os.path.exists(L.TEST_LIB_PATH), "build_variants/libbipymc_test.so missing: make -C bipymc_amd/csrc"
    return L.TEST_LIB_PATH


def test_alternative_kernel_paths_on_one_gpu():
    """Kernel paths that a small single-GPU run does not take by itself must reproduce the default one bit for bit,
    for every kernel shape.  They are selected through the library's ONE test variable, BPM_TEST_PATHS (sampler.hip: test_path):
    mode1 -- world_size > 1 launches one work item per LOCAL chain and filters by the chain's position in the shuffle order
    (inverse table); noplan -- header block and partner ids drawn inside the update kernel (what > 16384 chains per GPU use)
    instead of read from plan_kernel's records; noperm -- the shuffle bijection walked in the kernel instead of looked up;
    planall -- plan records whatever the number of chains; nohot -- the general instantiation instead of the specialised ones;
    wt8 -- round 2's two 8-byte write-through stores per lane instead of one 16-byte store; histchain -- the history append by chain
    index instead of in shuffle order (what fewer than 64 lanes per chain use); crslots -- level 1 of the CR reduction computed from the slots by
    cr_level1_kernel (what a rank of a world and the general kernel use) instead of inside the update kernels; lean -- ln_like of the current state
    re-evaluated from the own row and accepts counted per wavefront (what >= 49152 chains per GPU use) at any size; crnofold -- every generation's
    CR fold dispatched as cr_final_kernel instead of left to the next generation's first update launch (the consumer-side fold of round 5);
    and the operational switches BPM_DIRECT_QUEUE=0 (HIP stream launches) and BPM_QUEUE_INFLIGHT (a drain every few dispatches)."""
    import subprocess
    import sys
    code = r'''
import os, sys, numpy as np
sys.path.insert(0, os.getcwd())
from bipymc_amd import _lib as L
from bipymc_amd.engine import HipEngine
from bipymc_amd.utils import d100_gauss, banana_rv, mixture_nd
out = []
for spec, algo, N, kw in ((d100_gauss.Gauss_100D()._bpm_target_spec(), L.ALGO_DREAM, 96, dict(burnin_gen=6, n_cr_gen=2)),
                          (mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), L.ALGO_DREAM, 101, dict(burnin_gen=6, n_cr_gen=2, del_pairs=2)),
                          (mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), L.ALGO_DREAM, 9001, dict(burnin_gen=9, n_cr_gen=2)),   # 564 level-1 chunks
                          (d100_gauss.Gauss_100D()._bpm_target_spec(), L.ALGO_DREAM, 8192, dict(burnin_gen=11, n_cr_gen=2)),   # 512 level-1 chunks: the most the fold takes
                          (banana_rv.Banana_2D()._bpm_target_spec(), L.ALGO_DEMC, 77, dict(p_snooker=0.2))):
    tid, tp, d = spec
    e = HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=5, **kw)
    e.set_state(np.random.RandomState(0).normal(size=(N, d)) + 1.0)
    e.begin_run(); e.step(15)
    out.append(e.get_state()); out.append(np.array([e.stats()["local_n_accepted"]], dtype=float)); out.append(e.stats()["p_cr"])
np.save(sys.argv[1], np.concatenate([o.reshape(-1) for o in out]))
'''
    import tempfile
    res = []
    for paths, extra in (("", {}), ("nohot", {}), ("mode1", {}), ("noplan", {}), ("noperm", {}), ("mode1,noplan", {}), ("planall", {}),
                         ("planall,mode1", {}), ("", {"BPM_DIRECT_QUEUE": "0"}), ("nohot", {"BPM_DIRECT_QUEUE": "0"}),
                         ("", {"BPM_QUEUE_INFLIGHT": "3"}), ("wt8", {}), ("histchain", {}), ("wt8,histchain,nohot", {}), ("crslots", {}), ("lean", {}),
                         ("crslots,lean,mode1", {}), ("crnofold", {}), ("crnofold", {"BPM_DIRECT_QUEUE": "0"})):
        env = dict(os.environ)
        for k in ("BPM_TEST_PATHS", "BPM_DIRECT_QUEUE", "BPM_QUEUE_INFLIGHT"):
            env.pop(k, None)
        if paths:                 # (the product library does not read BPM_TEST_PATHS: the alternative paths exist in the test variant only --
            env["BPM_TEST_PATHS"] = paths      # whose default path thereby is compared with the product's as well)
            env["BPM_LIB_PATH"] = _test_lib_path()
        env.update(extra)
        with tempfile.TemporaryDirectory() as td:
            f = os.path.join(td, "o.npy")
            subprocess.check_call([sys.executable, "-c", code, f], env=env, cwd=os.path.join(os.path.dirname(__file__), ".."))
            res.append(np.load(f))
    for r in res[1:]:
        assert np.array_equal(res[0], r)


def test_cr_fold_inside_the_next_launch_equals_the_dispatched_fold_over_random_call_sequences():
    """Round 5: during DREAM's burn-in a generation's CR fold is not dispatched -- the next generation's first update launch folds the partial sums in every
    workgroup (kernels.h: PhaseArgs::cr_fold_part), the last generation of a step call and whatever cannot consume a pending fold get cr_final_kernel
    (sampler.hip: cr_pending).  Seeded random call sequences -- step calls of 1 ... 20 generations through and past a 60-generation burn-in, reads of the
    CR statistics and the state in between, a new run, the outlier check due every 7 generations -- on every kernel shape (64 / 16 / 4 / 1 lanes per chain,
    with and without cr_mid_kernel passes): p_cr, delta_m, n_cr_updates, state and ln-like after every call equal, bit for bit, what the test variant leaves
    with every fold dispatched (crnofold), with level 1 from the slots (crslots) and with the general kernel (nohot)."""
    import subprocess
    import sys
    import tempfile
    code = r'''
import os, sys, numpy as np
sys.path.insert(0, os.getcwd())
from bipymc_amd import _lib as L
from bipymc_amd.engine import HipEngine
from bipymc_amd.utils import d100_gauss, mixture_nd
out = []
cases = ((d100_gauss.Gauss_100D()._bpm_target_spec(), 2048, dict(burnin_gen=60, n_cr_gen=3)),
         (d100_gauss.Gauss_100D(dim=20)._bpm_target_spec(), 333, dict(burnin_gen=60, n_cr_gen=2)),
         (mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), 6000, dict(burnin_gen=60, n_cr_gen=3, outlier_every=7)),
         (mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), 40000, dict(burnin_gen=60, n_cr_gen=3)),          # 2500 level-1 sums: one cr_mid_kernel pass
         (mixture_nd.BimodeGauss_ND(2)._bpm_target_spec(), 3001, dict(burnin_gen=60, n_cr_gen=2)))
for ci, ((tid, tp, d), N, kw) in enumerate(cases):
    rs = np.random.RandomState(100 + ci)
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=77 + ci, keep_history=True, **kw)
    e.set_state(np.random.RandomState(ci).normal(size=(N, d)) + 0.5)
    e.begin_run()
    done = 0
    while done < 90:
        k = int(rs.choice([1, 1, 2, 3, 5, 8, 20]))
        e.step(k)
        done += k
        st = e.stats()
        out += [st["p_cr"], st["delta_m"], st["n_cr_updates"], np.array([st["local_n_accepted"], st["n_outlier_resets"]], dtype=float)]
        if rs.randint(0, 3) == 0:
            out += [e.get_state(), e.get_loglike()]
        if done > 30 and rs.randint(0, 8) == 0:
            e.begin_run()                      # (a new run_mcmc call: the generation counter of the run restarts, burn-in is on again)
    out += [e.get_state(), e.get_loglike()]
    e.close()
np.save(sys.argv[1], np.concatenate([np.asarray(o, dtype=float).reshape(-1) for o in out]))
'''
    res = []
    for paths in ("", "crnofold", "crslots", "nohot"):
        env = dict(os.environ)
        env.pop("BPM_TEST_PATHS", None)
        if paths:
            env["BPM_TEST_PATHS"] = paths
            env["BPM_LIB_PATH"] = _test_lib_path()
        with tempfile.TemporaryDirectory() as td:
            f = os.path.join(td, "o.npy")
            subprocess.check_call([sys.executable, "-c", code, f], env=env, cwd=os.path.join(os.path.dirname(__file__), ".."))
            res.append(np.load(f))
    for r in res[1:]:
        assert r.shape == res[0].shape and np.array_equal(res[0], r)


def test_outlier_check_reads_position_ordered_history_where_it_lies():
    """DREAM burn-in with the outlier check on a sampler that appends its history in shuffle order (fewer than 64 lanes per chain, one GPU): the
    state rows stay in position order and the check's kernels find a chain's rows through the rows' shuffle keys (outlier_row_keys), the ln-like rows
    are appended by chain while the check is due.  Against the same run with every row appended by chain (test path histchain): state, whole history,
    ln-like history, CR statistics, reset and accept counts equal bit for bit -- with chains parked far out (resets happen, the moment rebuild of a
    reset chain walks position-ordered rows), a partial history read in the middle (rows put back into chain order: mixed rows afterwards), the run
    going on past burn-in (rows appended by position with their ln-like by position again), d = 8 (4 lanes per chain) and d = 2 (one lane per chain)."""
    import subprocess
    import sys
    import tempfile
    code = r'''
import os, sys, numpy as np
sys.path.insert(0, os.getcwd())
from bipymc_amd import _lib as L
from bipymc_amd.engine import HipEngine
from bipymc_amd.utils import mixture_nd
out = []
for d, N in ((8, 4099), (2, 3001)):
    m = mixture_nd.BimodeGauss_ND(d)
    tid, tp, dd = m._bpm_target_spec()
    np.random.seed(3)
    x0 = m.rvs(N)
    x0[::97] = 25.0                      # parked in the far tail
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=dd, target_id=tid, target_params=tp, seed=9, burnin_gen=40, n_cr_gen=3, outlier_every=7)
    e.set_state(x0)
    e.begin_run()
    e.step(20)
    mid = e.get_history(0, 10)           # rows 0..9 back into chain order; the later rows stay as appended
    e.step(33)                           # checks at 21, 28, 35; burn-in ends at 40
    st = e.stats()
    assert st["n_outlier_resets"] >= N // 97, st["n_outlier_resets"]
    out += [mid, e.get_state(), e.get_history(), e.get_loglike_history(), e.get_loglike(), np.asarray(st["p_cr"]), np.asarray(st["delta_m"]),
            np.array([st["n_outlier_resets"], st["local_n_accepted"], st["local_n_rejected"]], dtype=float)]
    e.close()
np.save(sys.argv[1], np.concatenate([np.asarray(o, dtype=float).reshape(-1) for o in out]))
'''
    res = []
    for paths in ("", "histchain", "nohot"):
        env = dict(os.environ)
        for k in ("BPM_TEST_PATHS", "BPM_DIRECT_QUEUE", "BPM_QUEUE_INFLIGHT"):
            env.pop(k, None)
        if paths:
            env["BPM_TEST_PATHS"] = paths
            env["BPM_LIB_PATH"] = _test_lib_path()
        with tempfile.TemporaryDirectory() as td:
            f = os.path.join(td, "o.npy")
            subprocess.check_call([sys.executable, "-c", code, f], env=env, cwd=os.path.join(os.path.dirname(__file__), ".."))
            res.append(np.load(f))
    for r in res[1:]:
        assert np.array_equal(res[0], r)


@pytest.mark.parametrize("case,exchange", [("dream_gauss400", "replay"), ("dream_gauss400", "rows"), ("dream_gauss400", "dense"), ("dream_gauss900", "dense"),
                                           ("dream_gauss2500", "dense")])
def test_multi_rank_equals_single_rank_with_wide_rows(case, exchange):
    """d = 400: 8 coordinates per lane through the RCCL exchanges' kernels; d = 900 / 2500: the looped wide-row kernel (kernels_wide.h) as a rank
    of a world, dense exchange (the push exchange: tests/test_gpu_push.py); two emulated ranks."""
    _multi_rank_case(case, 2, exchange)


def test_wide_rows_have_no_replay_or_packed_rows_exchange():
    """Rows wider than 512 coordinates run on the looped kernel, which has no replay / packed-rows form: asking for those exchanges is an error that
    names the two that exist (push, dense) -- not a silent fall-back."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, d = d100_gauss.Gauss_100D(dim=600)._bpm_target_spec()
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=L.ALGO_DREAM, n_chains=16, dim=d, target_id=tid, target_params=tp, seed=1, rank=r, world_size=2, nccl_uid=uid, lib=L.load_test()) for r in range(2)]
    assert ranks[0].exchange_stats()["mode"] == "dense"
    for mode in ("replay", "rows"):
        with pytest.raises(L.BpmError, match="exchange by push"):
            ranks[0].set_exchange(mode=mode)
    ranks[0].set_exchange(mode="dense")
    for e in ranks:
        e.close()


@pytest.mark.parametrize("exchange", ["replay", "rows", "rows_overflow", "dense"])
@pytest.mark.parametrize("case", ["dream_gauss100", "dream_mix8", "demc_banana_snooker", "dream_gauss7_pairs2"])
@pytest.mark.parametrize("R", [2, 4])
def test_multi_rank_equals_single_rank_on_device(case, R, exchange):
    _multi_rank_case(case, R, exchange)


def _multi_rank_case(case, R, exchange):
    """The world_size > 1 device path (rank blocks of the exchange buffer, per-rank history / ln_like /
    Welford / accept counters, local-chain launch mode, CR statistics travelling in the gathered block)
    emulated with R handles on ONE GPU (bpm_local_group_step; the RCCL all-gather replaced by device
    copies): chain histories and p_cr must equal the single-rank run bit for bit.  `exchange`: the default accept-byte
    exchange with replay of the accepted proposals on the receiving ranks, the accepted-rows exchange, the same with a
    capacity of 2 rows (every chunk overflows, is rolled back to its checkpoint and repeated dense), and the dense
    all-gather."""
    import ctypes as C
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import banana_rv, d100_gauss, mixture_nd
    if case == "dream_gauss100":
        spec, algo, N, kw = d100_gauss.Gauss_100D()._bpm_target_spec(), L.ALGO_DREAM, 64, dict(burnin_gen=8, n_cr_gen=3)
    elif case == "dream_mix8":
        spec, algo, N, kw = mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), L.ALGO_DREAM, 48, dict(burnin_gen=8, n_cr_gen=3)
    elif case == "demc_banana_snooker":
        spec, algo, N, kw = banana_rv.Banana_2D()._bpm_target_spec(), L.ALGO_DEMC, 40, dict(p_snooker=0.3)
    elif case in ("dream_gauss400", "dream_gauss900", "dream_gauss2500"):       # 8 coordinates per lane / the looped wide-row kernel
        spec, algo, N, kw = d100_gauss.Gauss_100D(dim=int(case[11:]))._bpm_target_spec(), L.ALGO_DREAM, 32, dict(burnin_gen=6, n_cr_gen=2)
    else:
        spec, algo, N, kw = d100_gauss.Gauss_100D(dim=7)._bpm_target_spec(), L.ALGO_DREAM, 32, dict(burnin_gen=20, n_cr_gen=2, del_pairs=2)
    tid, tp, d = spec
    G = 14 if exchange != "rows_overflow" else 150        # 150: three chunks, so the capacity adapts after a rollback
    x0 = np.random.RandomState(3).normal(size=(N, d)) + 0.5
    one = HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, **kw)
    one.set_state(x0)
    one.begin_run(flip=0.4)
    one.step(G)
    H1 = one.get_history()                                    # (G+1, N, d)
    st1 = one.stats()

    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, rank=r, world_size=R,
                       nccl_uid=uid, lib=L.load_test(), **kw) for r in range(R)]
    for e in ranks:
        e.set_state(x0)
        e.begin_run(flip=0.4)
        e.set_exchange(mode=exchange.split("_")[0], cap=2 if exchange == "rows_overflow" else 0)
    arr = (C.c_void_p * R)(*[e._h for e in ranks])
    L.check(ranks[0].lib.bpm_local_group_step(arr, R, G), ranks[0].lib)
    xs = [e.exchange_stats() for e in ranks]
    assert all(x == xs[0] for x in xs)                                 # every rank took the same decisions
    n_sparse_gens = max(0, G - (kw.get("burnin_gen", 0) if algo == L.ALGO_DREAM else 0))     # CR adaptation runs dense
    assert xs[0]["mode"] == exchange.split("_")[0]
    if exchange == "replay":
        assert xs[0]["replay_gens"] == n_sparse_gens and xs[0]["chunks"] == 0
    elif exchange == "dense" or n_sparse_gens == 0:
        assert xs[0]["chunks"] == 0 and xs[0]["replay_gens"] == 0
    else:
        assert xs[0]["chunks"] >= 1 and xs[0]["replay_gens"] == 0
        assert (xs[0]["replays"] >= 1) == (exchange == "rows_overflow")
        if exchange == "rows_overflow":
            assert xs[0]["replays"] < xs[0]["chunks"] and xs[0]["cap"] > 2     # the capacity grew and later chunks fit
    HR = np.concatenate([e.get_history() for e in ranks], axis=1)      # ranks own contiguous id blocks (demc.py:39)
    assert HR.shape == H1.shape
    assert np.array_equal(HR, H1)
    for e in ranks:
        assert np.array_equal(e.get_state(), one.get_state())          # every replica is complete and identical
        st = e.stats()
        np.testing.assert_array_equal(st["p_cr"], st1["p_cr"])
        np.testing.assert_array_equal(st["n_cr_updates"], st1["n_cr_updates"])
    assert sum(e.stats()["local_n_accepted"] for e in ranks) == st1["local_n_accepted"]
    lls = np.concatenate([e.get_loglike() for e in ranks])
    assert np.array_equal(lls, one.get_loglike())
    with pytest.raises(L.BpmError):
        ranks[0].step(1)                                               # local-group ranks are not driven individually


def test_example_line_fit_host_callback():
    """examples/ex_para_fit.py (the reference's examples/ex_para_fit.py:39-110 scenario): a Python lnprob
    with ln_kwargs and a -inf prior, through both drop-in classes."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ex_para_fit", os.path.join(os.path.dirname(__file__), "..", "examples", "ex_para_fit.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    from bipymc_amd import DeMcMpi, DreamMpi
    for cls in (DreamMpi, DeMcMpi):
        s, est, sig, truth = ex.run(cls, n_chains=12, n=12 * 2501)
        assert not s.uses_device_target
        # posterior of 50 noisy points: the truth lies within ~3 posterior sigmas
        assert np.all(np.abs(est - np.array(truth)) < 3.5 * sig + 0.05), (est, sig, truth)
        assert 0.02 < s.acceptance_fraction < 0.7


def test_serial_api_demc_class():
    """bipymc_amd.samplers.DeMc == the reference's serial `DeMc` surface (samplers.py:237-336;
    examples/ex_line_fit.py:77 style): run_mcmc(n, theta_0), param_est, super_chain, acceptance_fraction."""
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import banana_rv
    np.random.seed(3)
    banana = banana_rv.Banana_2D()
    s = DeMc(banana.ln_like, n_chains=64)
    s.run_mcmc(64 * 3001, np.zeros(2), varepsilon=1e-4)
    mean, std, chain = s.param_est(n_burn=64 * 1000)
    assert s.super_chain.shape == (64 * 3001, 2) and chain.shape == (64 * 2001, 2)
    assert abs(mean[0]) < 0.1 and abs(mean[1] - 1.16125) < 0.1                 # SURVEY a13 analytic moments
    assert abs(std[0] ** 2 - 1.3225) < 0.15
    assert 0.1 < s.acceptance_fraction < 0.6
    assert s.n_accepted + s.n_rejected == 64 * 3000 + 1                        # samplers.py:30-31: starts at 1/0
    assert np.array_equal(s.super_chain[5::64], s.am_chains[5].chain) and np.array_equal(s.current_pos, s.am_chains[0].chain[-1])
    # a Python callable with kwargs takes the host path; a second run re-initialises the chains (samplers.py:266-267)
    t = DeMc(lambda th, s2=1.0: -0.5 * float(np.sum(th ** 2)) / s2, n_chains=16, ln_kwargs={"s2": 4.0})
    t.run_mcmc(16 * 1501, np.zeros(3), varepsilon=1e-2)
    m, sd, _ = t.param_est(16 * 500)
    assert np.all(np.abs(m) < 0.35) and np.all(np.abs(sd - 2.0) < 0.35)
    acc1 = t.n_accepted
    t.run_mcmc(16 * 11, np.ones(3))
    assert t.super_chain.shape == (16 * 11, 3) and t.n_accepted >= acc1
    with pytest.raises(NotImplementedError):
        t.run_mcmc(100, np.zeros(3), delayed_accept=False)


@pytest.mark.parametrize("d", [6, 600])
def test_serial_demc_class_device_and_host_paths_equal_the_oracle(d):
    """bipymc_amd.samplers.DeMc with a fixed seed, run twice: on the bound ln_like of the shipped Gauss_100D (recognised: evaluated on the device, the
    generation loop is bpm_step on BPM_ALGO_DEMC_SYNC) and on the same density behind a plain Python function (the host path: one bpm_propose / bpm_commit
    round per generation, the commit kernel banks into x_next) -- d = 6 (16 lanes per chain) and d = 600 (the looped wide-row kernels).  The two runs and
    OracleSampler(ALGO_DEMC_SYNC) started from the class's own jittered start (history row 0) with the class's run options (samplers.py:283: jitter std
    sqrt(varepsilon * 1e-3), no shuffle) give the same chains: accept counts equal, the two paths 1e-11 / 1e-13 apart (two summation orders of one
    formula), each 1e-10 / 1e-12 from the oracle (tests/test_gpu_shipped_path.py: floats after G generations).  varepsilon = 1e-21 with
    inflate = 1e21 starts the chains with unit variance (samplers.py:255-259) and makes the per-generation jitter 1e-12, DREAM's default: the
    float32 Box-Muller of a larger one would be the difference the test sees."""
    from bipymc_amd.samplers import DeMc
    from bipymc_amd.utils import d100_gauss
    from oracle import sampler_ref as R
    N, gens, seed = 16, 40, 4242
    tgt = d100_gauss.Gauss_100D(rho=0.3, dim=d)
    theta_0 = np.linspace(-1.0, 1.0, d)

    def py_ll(theta):
        return tgt.ln_like(theta)

    runs = []
    for fn, on_device in ((tgt.ln_like, True), (py_ll, False)):
        s = DeMc(fn, n_chains=N, seed=seed)
        s.run_mcmc(N * (gens + 1), theta_0, varepsilon=1e-21, inflate=1e21)
        assert s._device_target == on_device
        assert s.super_chain.shape == (N * (gens + 1), d)
        runs.append((s.super_chain, s.n_accepted, s.n_rejected))
        s._engine.close()          # (the class refers to itself through its frozen ln_like_fn: left alone, its device memory would wait for a garbage collection)
    (dev, acc_dev, rej_dev), (host, acc_host, rej_host) = runs
    X0 = dev[:N]
    assert np.array_equal(X0, host[:N]) and np.all(np.std(X0, axis=0) > 0.3)       # the same jittered start, of unit variance
    np.testing.assert_allclose(dev, host, rtol=1e-11, atol=1e-13)
    assert acc_dev == acc_host and rej_dev == rej_host
    params = R.gauss_equicorr_params(0.3, np.sqrt(np.arange(d) + 1.0))
    ora = R.OracleSampler(R.ALGO_DEMC_SYNC, N, d, R.TARGET_GAUSS_EQUICORR, params, seed)
    ora.set_state(X0)
    ora.run(gens, flip=0.0, shuffle=False, epsilon=float(np.sqrt(1e-21 * 1e-3)), gamma=None)
    assert 0 < ora.local_n_accepted < N * gens
    assert acc_dev == 1 + ora.local_n_accepted and rej_dev == ora.local_n_rejected - 1          # samplers.py:30-31: the class starts at 1 / 0
    np.testing.assert_allclose(dev, ora.super_chain(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(host, ora.super_chain(), rtol=1e-10, atol=1e-12)


def test_posterior_moments_at_baseline_sizes():
    """'Posterior moments within 1 % of reference' (BASELINE.json north_star) at the BASELINE sizes, PER COORDINATE (the pooled form
    hid a per-coordinate spread of 0.988 ... 1.016 over 1200 generations, and 3.5 % was what this test allowed): every coordinate's variance within 1 %
    of the analytic value and every coordinate's mean within 0.01 sigma, with the batch-means standard error of the worst coordinate at most a third of
    the tolerance -- over 40 000 post-burn-in generations of cfg2 (one second with per-generation population sums instead of a history), from exact
    draws of the target AND from the reference's own start (theta_0 = 0, varepsilon = 1e-6; chain.py:25-27, tests/test_100dgauss.py:105-110) behind a
    3000-generation transient; the same gate for cfg3 and for cfg5 (its per-GPU share and whole).  The gate is bench.py's (batch_moment_gate): what the
    JSON line reports as posterior.gate is what is asserted here."""
    import bench
    for start in ("exact", "reference"):
        g = bench.posterior_gate(0, start=start)
        assert g["generations"] == bench.POSTERIOR_GATE_GENS and g["batches"] == bench.GATE_BATCHES
        assert g["gate_pass"], g
        assert 0.99 <= g["var_ratio_min"] <= g["var_ratio_max"] <= 1.01 and g["max_abs_mean_over_sigma"] <= 0.01, g
        assert g["mcse_var_ratio_max"] <= 0.01 / 3 and g["mcse_mean_over_sigma_max"] <= 0.01 / 3, g
        assert 0.15 < g["acceptance_fraction"] < 0.20                    # (cfg2's DREAM: 0.172-0.176)
    others = bench.posterior_gates_other_configs(0)
    assert len(others) == 3
    for g in others:
        assert "error" not in g and g["gate_pass"], g
        assert 0.99 <= g["var_ratio_min"] <= g["var_ratio_max"] <= 1.01 and g["max_abs_mean_over_sigma"] <= 0.01, g


def test_outlier_reset_keeps_the_modes_at_cfg5_share():
    """cfg5 (one GPU's share of the 8-D mixture, N = 32768) with CR adaptation and the outlier reset on: chains parked in the far tail are reset, everybody
    ends in one of the two modes, the mode weights are preserved and the per-axis variance inside each mode is that of the 2-D reference target
    (dblgauss_rv.py:11-32: sigma = 0.25)."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import mixture_nd
    np.random.seed(5)
    m = mixture_nd.BimodeGauss_ND(8)
    tid, tp, d = m._bpm_target_spec()
    N = 32768
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=3, burnin_gen=300, n_cr_gen=50,
                  outlier_every=50)
    x0 = m.rvs(N)
    x0[:7] = 40.0                                                              # a few chains parked in the far tail
    e.set_state(x0)
    e.begin_run(); e.step(600)
    st = e.stats()
    assert st["n_outlier_resets"] >= 7
    X = e.get_state()
    in0 = np.all(np.abs(X) < 1.6, axis=1)                                      # sigma = 0.25 per axis: 6.4 sigma boxes
    in2 = np.all(np.abs(X - 2.0) < 1.6, axis=1) & ~in0
    assert in0.sum() + in2.sum() == N                                          # everybody sits in one of the two modes
    assert abs(in0.mean() - 0.25) < 0.02                                       # mode weights preserved (w = 0.25 / 0.75)
    assert abs(X[in2].var(axis=0).mean() / 0.0625 - 1) < 0.02 and abs(X[in0].var(axis=0).mean() / 0.0625 - 1) < 0.03
    e.close()


def test_vectorized_callback_and_device_moments():
    from bipymc_amd import DreamMpi
    calls = []

    def ll_batch(thetas, s2=1.0):
        thetas = np.atleast_2d(thetas)
        calls.append(thetas.shape[0])
        return -0.5 * np.sum(thetas ** 2, axis=1) / s2

    a = DreamMpi(ll_batch, np.zeros(4), n_chains=32, seed=4, burnin_gen=50, n_cr_gen=10, vectorized=True, ln_kwargs={"s2": 2.0})
    b = DreamMpi(lambda th, s2=1.0: float(-0.5 * np.sum(th ** 2) / s2), np.zeros(4), n_chains=32, seed=4, burnin_gen=50,
                 n_cr_gen=10, ln_kwargs={"s2": 2.0})
    a.run_mcmc(32 * 301)
    b.run_mcmc(32 * 301)
    assert len(calls) == 1 + 2 * 300 and max(calls) == 32              # one call per half generation
    np.testing.assert_allclose(a.param_est(0)[2], b.param_est(0)[2], rtol=1e-12, atol=1e-14)
    mean, std, _ = a.param_est(32 * 100)
    m2, s2 = a.param_est_moments(32 * 100)
    np.testing.assert_allclose(m2, mean, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(s2, std, rtol=1e-9)
    assert np.all(np.abs(std - np.sqrt(2.0)) < 0.25)


@pytest.mark.parametrize("dim,N,G", [(100, 8192, 24), (7, 65536, 44)])
def test_large_history_transfer_equals_row_by_row(dim, N, G):
    """bpm_get_history switches to the multi-threaded pinned-staging copy above 128 MB; it must return exactly what
    generation-by-generation calls (the plain path) return, also when rows are padded on the device (odd dim)."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, d = d100_gauss.Gauss_100D(dim=dim)._bpm_target_spec()
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=5, burnin_gen=0)
    e.set_state(np.random.RandomState(1).normal(size=(N, d)))
    e.begin_run()
    e.step(G)
    H = e.get_history()
    assert H.shape == (G + 1, N, d) and H.nbytes >= 128 << 20
    for g in range(G + 1):
        assert np.array_equal(H[g], e.get_history(g, g + 1)[0]), g
    assert np.array_equal(H[-1], e.get_state())
    e.close()


def test_long_run_crosses_many_table_chunks_and_stays_stationary():
    """20000 generations in one run_mcmc-sized step: 313 chunks of shuffle tables / plan records, a 33 GB history written
    by streaming stores, generation counters far beyond the 16-bit range.  Started from exact draws of the target the
    pooled moments of ALL rows must stay at the analytic values, and the last row must still be a plausible draw."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    np.random.seed(11)
    g = d100_gauss.Gauss_100D()
    tid, tp, d = g._bpm_target_spec()
    N, G = 2048, 20000
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=9, burnin_gen=0)
    e.set_state(g.rvs(N))
    e.begin_run()
    e.step(G)
    st = e.stats()
    assert st["k_gen"] == G and st["history_rows"] == G + 1
    assert st["local_n_accepted"] + st["local_n_rejected"] == N * G + 1
    assert 0.1 < st["local_n_accepted"] / (N * G) < 0.35
    cnt, s1, s2, sh = e.reduce_moments(0)
    assert cnt == N * (G + 1)
    mean, var = sh + s1 / cnt, s2 / cnt - (s1 / cnt) ** 2
    sig2 = np.arange(d) + 1.0
    assert np.max(np.abs(mean) / np.sqrt(sig2)) < 0.02
    assert abs(np.mean(var / sig2) - 1) < 0.01 and np.max(np.abs(var / sig2 - 1)) < 0.03
    X = e.get_state()
    assert abs(np.mean(X.var(axis=0) / sig2) - 1) < 0.05                      # the final population alone (2048 draws)
    assert np.array_equal(e.get_history(G, G + 1)[0], X)
    e.close()


@pytest.mark.parametrize("exchange", ["replay", "rows"])
def test_eight_rank_world_equals_single_rank(exchange):
    """The shape the scaling bench runs (8 ranks, the 100-D Gaussian, one wavefront per chain, plan records, the sharded
    steady-state instantiation, replay of seven other ranks' accepted proposals), emulated on one GPU at 128 chains per
    rank: 60 generations including a DREAM burn-in with CR adaptation must equal the single-rank run bit for bit."""
    import ctypes as C
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    g = d100_gauss.Gauss_100D()
    tid, tp, d = g._bpm_target_spec()
    R, N, G = 8, 1024, 60
    kw = dict(burnin_gen=12, n_cr_gen=3)
    np.random.seed(8)
    x0 = g.rvs(N)
    one = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=21, **kw)
    one.set_state(x0)
    one.begin_run()
    one.step(G)
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=21, rank=r, world_size=R,
                       nccl_uid=uid, lib=L.load_test(), **kw) for r in range(R)]
    for e in ranks:
        e.set_state(x0)
        e.begin_run()
        e.set_exchange(mode=exchange)
    arr = (C.c_void_p * R)(*[e._h for e in ranks])
    L.check(ranks[0].lib.bpm_local_group_step(arr, R, G), ranks[0].lib)
    HR = np.concatenate([e.get_history() for e in ranks], axis=1)
    assert np.array_equal(HR, one.get_history())
    for e in ranks:
        assert np.array_equal(e.get_state(), one.get_state())
        np.testing.assert_array_equal(e.stats()["p_cr"], one.stats()["p_cr"])
    assert sum(e.stats()["local_n_accepted"] for e in ranks) == one.stats()["local_n_accepted"]
    assert ranks[0].exchange_stats()["replay_gens" if exchange == "replay" else "chunks"] > 0


def test_config4_shape_eight_ranks_equal_single_rank():
    """BASELINE config 4 itself -- 65536 chains of the 100-D Gaussian as 8 ranks of 8192 -- emulated on one GPU: 130
    generations (40 of burn-in with CR adaptation and the dense exchange, then the replay exchange with rank-local
    records) leave every replica, p_cr and the accept counts exactly where the single-rank run of 65536 chains ends."""
    import ctypes as C
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    g = d100_gauss.Gauss_100D()
    tid, tp, d = g._bpm_target_spec()
    R, N, G = 8, 65536, 130
    kw = dict(burnin_gen=40, n_cr_gen=10)
    np.random.seed(4)
    x0 = g.rvs(N)
    one = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=5, keep_history=False, **kw)
    one.set_state(x0)
    one.begin_run()
    one.step(G)
    X1, st1 = one.get_state(), one.stats()
    one.close()
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=5, rank=r, world_size=R,
                       nccl_uid=uid, lib=L.load_test(), **kw) for r in range(R)]
    for e in ranks:
        e.set_state(x0)
        e.begin_run()
    arr = (C.c_void_p * R)(*[e._h for e in ranks])
    L.check(ranks[0].lib.bpm_local_group_step(arr, R, G), ranks[0].lib)
    assert ranks[0].exchange_stats()["mode"] == "replay" and ranks[0].exchange_stats()["replay_gens"] == G - 40
    for e in ranks:
        assert np.array_equal(e.get_state(), X1)
        np.testing.assert_array_equal(e.stats()["p_cr"], st1["p_cr"])
    assert sum(e.stats()["local_n_accepted"] for e in ranks) == st1["local_n_accepted"]
    for e in ranks:
        e.close()


@pytest.mark.parametrize("exchange", ["dense", "replay"])
def test_cr_slots_are_fresh_when_adaptation_resumes_in_a_world(exchange):
    """The chains' CR slots (delta | CR index) are written only by generations whose reduction reads them -- adapting, level 1 not summed inside the
    update kernel (round 4: the steady state had stored "no statistic" with every update).  Burn-in restarts with every run (demc.py:78, dream.py:92):
    three runs of 4 adapting + 9 steady generations in a world of two emulated ranks (level 1 from the slots, which hold the LAST adapting
    generation's values all through the steady part and must all be rewritten before the next reduction reads them) against the single-rank run
    (level 1 inside its update kernels, slots never written): p_cr, delta_m, n_cr_updates and every replica equal bit for bit."""
    import ctypes as C
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss, mixture_nd
    for spec, N in ((mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), 96), (d100_gauss.Gauss_100D()._bpm_target_spec(), 64)):
        tid, tp, d = spec
        kw = dict(burnin_gen=4, n_cr_gen=1)
        x0 = np.random.RandomState(5).normal(size=(N, d)) + 0.5
        one = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=13, **kw)
        one.set_state(x0)
        uid = b"BPMLOCAL" + bytes(120)
        ranks = [HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=13, rank=r, world_size=2, nccl_uid=uid, lib=L.load_test(), **kw)
                 for r in range(2)]
        arr = (C.c_void_p * 2)(*[e._h for e in ranks])
        for e in ranks:
            e.set_state(x0)
        for run in range(3):
            one.begin_run()
            one.step(13)
            for e in ranks:
                e.begin_run()
                e.set_exchange(mode=exchange, cap=0)
            L.check(ranks[0].lib.bpm_local_group_step(arr, 2, 13), ranks[0].lib)
            st1 = one.stats()
            assert np.all(np.asarray(st1["n_cr_updates"]) > 0)
            for e in ranks:
                st = e.stats()
                np.testing.assert_array_equal(st["p_cr"], st1["p_cr"])
                np.testing.assert_array_equal(st["delta_m"], st1["delta_m"])
                np.testing.assert_array_equal(st["n_cr_updates"], st1["n_cr_updates"])
                assert np.array_equal(e.get_state(), one.get_state())
        for e in ranks + [one]:
            e.close()


@pytest.mark.parametrize("R", [2, 4])
def test_outlier_reset_multi_rank_equals_single_rank(R):
    """The outlier-chain reset with world_size > 1 -- omega of the local chains, all-gather of the (omega | ln_like) blocks,
    quartiles / best chain / reset on every rank's replica -- emulated with R handles on one GPU: histories, p_cr and the
    number of resets equal the single-rank run bit for bit (the reset also repairs the owner's last history row, ln_like
    cache and Welford moments, which the following CR statistics depend on)."""
    import ctypes as C
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import mixture_nd
    m = mixture_nd.BimodeGauss_ND(8)
    tid, tp, d = m._bpm_target_spec()
    N, G = 64, 34
    kw = dict(burnin_gen=30, n_cr_gen=3, outlier_every=5)
    np.random.seed(12)
    x0 = m.rvs(N)
    x0[[3, 17, 40, 63]] = 30.0                      # parked in the far tail, on different ranks
    one = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=6, **kw)
    one.set_state(x0)
    one.begin_run()
    one.step(G)
    st1 = one.stats()
    assert st1["n_outlier_resets"] >= 4
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=6, rank=r, world_size=R,
                       nccl_uid=uid, lib=L.load_test(), **kw) for r in range(R)]
    for e in ranks:
        e.set_state(x0)
        e.begin_run()
    arr = (C.c_void_p * R)(*[e._h for e in ranks])
    L.check(ranks[0].lib.bpm_local_group_step(arr, R, G), ranks[0].lib)
    HR = np.concatenate([e.get_history() for e in ranks], axis=1)
    assert np.array_equal(HR, one.get_history())
    assert np.array_equal(np.concatenate([e.get_loglike_history() for e in ranks], axis=1), one.get_loglike_history())
    for e in ranks:
        st = e.stats()
        assert np.array_equal(e.get_state(), one.get_state())
        assert st["n_outlier_resets"] == st1["n_outlier_resets"]
        np.testing.assert_array_equal(st["p_cr"], st1["p_cr"])
        np.testing.assert_array_equal(st["delta_m"], st1["delta_m"])


def test_config5_as_stated_full_size():
    """BASELINE config 5 as it is written: DREAM, 8-D bimodal mixture, 262144 chains as 8 ranks of 32768, CR adaptation and
    outlier-chain detection ON.  (a) the 8-rank world, emulated on one GPU, ends exactly where the single-rank run of
    262144 chains ends (state, p_cr, resets, accept counts); (b) size-independent properties of that run: every parked
    chain was reset, everybody sits in one of the two modes, mode weights and within-mode variances are the target's."""
    import ctypes as C
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import mixture_nd
    m = mixture_nd.BimodeGauss_ND(8)
    tid, tp, d = m._bpm_target_spec()
    R, N, G = 8, 262144, 260
    kw = dict(burnin_gen=110, n_cr_gen=20, outlier_every=50)
    np.random.seed(15)
    x0 = m.rvs(N)
    parked = np.arange(0, N, 4099)                  # 64 chains spread over all ranks, far in the tail
    x0[parked] = 25.0
    one = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=31, **kw)
    one.set_state(x0)
    one.begin_run()
    one.step(G)
    X1, st1 = one.get_state(), one.stats()
    assert st1["history_rows"] == G + 1 and st1["local_n_accepted"] + st1["local_n_rejected"] == N * G + 1
    assert st1["n_outlier_resets"] >= parked.size
    assert abs(st1["p_cr"].sum() - 1.0) < 1e-12 and np.all(st1["n_cr_updates"] > 0)
    in0 = np.all(np.abs(X1) < 1.6, axis=1)
    in2 = np.all(np.abs(X1 - 2.0) < 1.6, axis=1) & ~in0
    assert in0.sum() + in2.sum() == N
    assert abs(in0.mean() - 0.25) < 0.01
    # (the reset rule moves low-density chains to the best chain ON PURPOSE -- it is a burn-in device and not reversible: with
    # it the within-mode variance sits ~2 % low at the end of burn-in, in the oracle too, and relaxes afterwards; 3 % here)
    assert abs(X1[in2].var(axis=0).mean() / 0.0625 - 1) < 0.03 and abs(X1[in0].var(axis=0).mean() / 0.0625 - 1) < 0.03
    assert np.array_equal(one.get_history(G, G + 1)[0], X1)
    one.close()
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=31, rank=r, world_size=R,
                       nccl_uid=uid, lib=L.load_test(), **kw) for r in range(R)]
    for e in ranks:
        e.set_state(x0)
        e.begin_run()
    arr = (C.c_void_p * R)(*[e._h for e in ranks])
    L.check(ranks[0].lib.bpm_local_group_step(arr, R, G), ranks[0].lib)
    for e in ranks:
        st = e.stats()
        assert np.array_equal(e.get_state(), X1)
        assert st["n_outlier_resets"] == st1["n_outlier_resets"]
        np.testing.assert_array_equal(st["p_cr"], st1["p_cr"])
    assert sum(e.stats()["local_n_accepted"] for e in ranks) == st1["local_n_accepted"]
    for e in ranks:
        e.close()


def test_warm_start_with_host_callback_and_outlier_check(tmp_path):
    """after a warm start with a Python ln_like_fn the ln-like history of the loaded rows is unknown (the reference's
    checkpoint stores no log-likes, chain.py:59-70).  Those rows are NaN on the device, the row of the current state is filled
    by bpm_set_loglike, and the outlier check averages over the rows it knows: a chain parked in the tail is still found and
    reset, nothing turns NaN."""
    from bipymc_amd import DreamMpi
    f = str(tmp_path / "ck.npz")

    def ll(theta):
        return float(-0.5 * np.sum(theta ** 2))

    a = DreamMpi(ll, np.zeros(3), n_chains=16, seed=8, burnin_gen=400, n_cr_gen=5, h5_file=f)
    a.run_mcmc(16 * 21)
    a.save_state(f)
    rows = a.param_est(0)[2].shape[0]
    # corrupt one chain of the checkpoint: far in the tail at the last row
    with np.load(f) as z:
        arrays = {k: z[k] for k in z.files}
    arrays["chains/chain_id_5"] = arrays["chains/chain_id_5"].copy()
    arrays["chains/chain_id_5"][-1] = 40.0
    np.savez_compressed(f, **arrays)
    b = DreamMpi(ll, None, n_chains=16, dim=3, seed=8, burnin_gen=400, n_cr_gen=5, h5_file=f, warm_start=True, outlier_every=4)
    assert not b.uses_device_target
    assert np.allclose(b.am_chains[5].current_pos, 40.0)
    b.run_mcmc(16 * 13)                                   # 12 generations: outlier checks at 4, 8, 12
    st = b._engine.stats()
    assert st["n_outlier_resets"] >= 1
    full = b.param_est(0)[2]
    assert full.shape[0] == rows + 16 * 12 and np.all(np.isfinite(full))
    assert np.all(np.abs(b._engine.get_state()) < 10.0)   # the parked chain restarted from the best one
    assert np.all(np.isfinite(b._engine.get_loglike()))


@pytest.mark.parametrize("R", [16, 24])
def test_many_ranks_sorted_records_and_fallback(R):
    """16 ranks is the most the owner-sorted record table serves (MAX_SEG); with more the records stay by position, the ranks launch
    one item per local chain and a replay wavefront per position (round 1's path).  Both equal the single-rank run bit for bit."""
    import ctypes as C
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    g = d100_gauss.Gauss_100D()
    tid, tp, d = g._bpm_target_spec()
    N, G = 24 * 16, 70                                   # crosses a table window (64 generations)
    kw = dict(burnin_gen=6, n_cr_gen=2)
    np.random.seed(2)
    x0 = g.rvs(N)
    one = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=3, **kw)
    one.set_state(x0)
    one.begin_run()
    one.step(G)
    uid = b"BPMLOCAL" + bytes(120)
    ranks = [HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=3, rank=r, world_size=R,
                       nccl_uid=uid, lib=L.load_test(), **kw) for r in range(R)]
    for e in ranks:
        e.set_state(x0)
        e.begin_run()
    arr = (C.c_void_p * R)(*[e._h for e in ranks])
    L.check(ranks[0].lib.bpm_local_group_step(arr, R, G), ranks[0].lib)
    assert np.array_equal(np.concatenate([e.get_history() for e in ranks], axis=1), one.get_history())
    for e in ranks:
        assert np.array_equal(e.get_state(), one.get_state())
        np.testing.assert_array_equal(e.stats()["p_cr"], one.stats()["p_cr"])
    assert sum(e.stats()["local_n_accepted"] for e in ranks) == one.stats()["local_n_accepted"]
    assert ranks[0].exchange_stats()["replay_gens"] == G - 6


@pytest.mark.parametrize("case", ["dream_gauss100", "dream_mix8_outlier", "demc_banana_snooker", "dream_gauss100_big", "dream_gauss100_wide"])
def test_direct_queue_equals_stream_launches(case):
    """The generation loop of a single-GPU sampler is dispatched by AQL packets the library writes into its own queue
    (bipymc_amd/csrc/aql_queue.h).  In the steady state those packets carry the acquire fence only and the update kernel writes what
    its successor reads with agent-scope stores (sampler.hip: Dispatch::update_fence); launching the same kernels on the HIP stream, or
    through the queue with a HIP stream's acquire + release on every packet, must give the same bits: state, ln-like, the whole
    history, CR statistics, accept counters.  The runs cross a table window (64 generations), grow the history while the queue is
    busy (no reservation), pass through burn-in with the outlier check (HIP-stream sections between drains) and call the timed entry
    point; the "wide" case rewrites more than 4 MiB of state per half generation (the size from which the packets keep the release)."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import banana_rv, d100_gauss, mixture_nd
    if case == "dream_gauss100":
        spec, algo, N, kw, G = d100_gauss.Gauss_100D()._bpm_target_spec(), L.ALGO_DREAM, 512, dict(burnin_gen=20, n_cr_gen=4), 150
    elif case == "dream_gauss100_big":
        spec, algo, N, kw, G = d100_gauss.Gauss_100D()._bpm_target_spec(), L.ALGO_DREAM, 8192, dict(burnin_gen=30, n_cr_gen=4), 100
    elif case == "dream_gauss100_wide":
        spec, algo, N, kw, G = d100_gauss.Gauss_100D()._bpm_target_spec(), L.ALGO_DREAM, 49152, dict(burnin_gen=4, n_cr_gen=2), 14
    elif case == "dream_mix8_outlier":
        spec, algo, N, kw, G = (mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), L.ALGO_DREAM, 20000,
                                dict(burnin_gen=60, n_cr_gen=4, del_pairs=2, outlier_every=20), 140)
    else:
        spec, algo, N, kw, G = banana_rv.Banana_2D()._bpm_target_spec(), L.ALGO_DEMC, 4099, dict(p_snooker=0.2), 200
    tid, tp, d = spec
    X0 = np.random.RandomState(3).normal(size=(N, d)) + 1.0
    res, stats = [], []
    for direct, fence in ((True, -1), (False, -1), (True, 3)):
        e = HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=11, **kw)
        ls = e.launch_stats()
        assert ls["has_queue"], "no direct AQL queue on this box: " + str(ls)
        assert not ls["coherent_state"] and ls["fence"] == "acquire", ls      # (ordinary memory, release-less steady state)
        with pytest.raises(L.BpmError):
            e.set_launch_path(True, 0)                                        # fence-less packets are not part of this library
        e.set_launch_path(direct, fence)
        e.set_state(X0)
        e.begin_run()
        before = e.launch_stats()
        e.step(G // 2)
        ms, nl = e.step_timed(G - G // 2 - 3)
        e.step(3)
        after = e.launch_stats()
        if direct:
            assert after["direct"] - before["direct"] == 2 * G and after["stream"] == before["stream"]
            # a burn-in-free tail: the timed call's launches are all update kernels (2 per generation, first to last)
            assert nl == 2 * (G - G // 2 - 3) - 1 and 0.0 < ms < 1e3
        else:
            assert after["stream"] - before["stream"] == 2 * G and after["direct"] == before["direct"]
        st = e.stats()
        res.append((e.get_state(), e.get_loglike(), e.get_history(0, G + 1), e.get_loglike_history(0, G + 1),
                    np.asarray(st["p_cr"]), np.asarray(st["delta_m"]), np.asarray(st["n_cr_updates"])))
        stats.append((st["local_n_accepted"], st["local_n_rejected"], st["n_outlier_resets"]))
        e.close()
    for r, s in zip(res[1:], stats[1:]):
        for a, b in zip(res[0], r):
            assert np.array_equal(a, b)
        assert s == stats[0]
    if case == "dream_mix8_outlier":
        assert stats[0][2] >= 0


def test_release_fence_is_needed_on_ordinary_memory():
    """Why the steady-state packets may drop the release fence only together with agent-scope stores: on ordinary device memory a
    dependent chain of kernels with acquire-only packets and PLAIN stores reads stale blocks (eight XCDs with an L2 each).  The
    probe must FAIL there; the hardware-coherent memory type of round 2's experiment is not compiled into the product library
    (asking for it is an error)."""
    import subprocess
    import sys
    code = ("import ctypes as C, os, sys; sys.path.insert(0, os.getcwd()); from bipymc_amd import _lib as L; lib = L.load_test(); w = C.c_int64(-2); "
            "rc = lib.bpm_debug_coherence_probe(0, 1, C.byref(w)); L.check(lib.bpm_debug_coherence_probe(0, 0, C.byref(w)), lib); print(rc, w.value)")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(os.path.dirname(__file__), ".."), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rc_coherent, ordinary_wrong = (int(v) for v in out.stdout.split()[-2:])
    assert rc_coherent != 0, "the experimental memory type must not be reachable in the product build"
    assert ordinary_wrong > 0, "ordinary device memory passed the probe: it no longer discriminates (%d)" % ordinary_wrong


def test_failed_queue_is_quiesced_or_buffers_are_leaked():
    """After a drain of the library's own queue ran into its limit, bpm_destroy must not free buffers that kernels on that queue may still
    use: it inactivates the queue (then frees), and if that is refused it leaks the buffers and says so.  Both in child
    processes: the device's queue is unusable for the rest of a process once it has failed."""
    import subprocess
    import sys
    code = r'''
import os, sys, numpy as np
sys.path.insert(0, os.getcwd())
from bipymc_amd import _lib as L
from bipymc_amd.engine import HipEngine
from bipymc_amd.utils import d100_gauss
tid, tp, d = d100_gauss.Gauss_100D()._bpm_target_spec()
refuse = int(sys.argv[1])
e = HipEngine(algo=L.ALGO_DREAM, n_chains=512, dim=d, target_id=tid, target_params=tp, seed=1, burnin_gen=0)
e.set_state(np.random.RandomState(0).normal(size=(512, d)))
e.begin_run(); e.step(20)
assert e.launch_stats()["direct"] == 40
L.check(e.lib.bpm_debug_fail_queue(e._h, refuse), e.lib)
try:
    e.close()
    print("DESTROY ok")
except L.BpmError as err:
    print("DESTROY error:", err)
# the process goes on: a new sampler launches on its HIP stream (the device's queue is dead) and is right
e2 = HipEngine(algo=L.ALGO_DREAM, n_chains=512, dim=d, target_id=tid, target_params=tp, seed=1, burnin_gen=0)
e2.set_state(np.random.RandomState(0).normal(size=(512, d)))
e2.begin_run(); e2.step(20)
ls = e2.launch_stats()
print("SECOND", ls["direct"] - 40, ls["stream"], float(e2.get_state().sum()))
e2.close()
'''
    root = os.path.join(os.path.dirname(__file__), "..")
    sums = []
    for refuse in (0, 1):
        out = subprocess.run([sys.executable, "-c", code, str(refuse)], cwd=root, capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, BPM_LIB_PATH=_test_lib_path()))          # (bpm_debug_fail_queue: a hook of the test variant)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        if refuse:
            assert "DESTROY error:" in out.stdout and "leaked" in out.stdout, out.stdout
        else:
            assert "DESTROY ok" in out.stdout, out.stdout
        second = [ln for ln in out.stdout.splitlines() if ln.startswith("SECOND")][0].split()
        assert int(second[1]) == 0 and int(second[2]) == 40, second          # all 40 update launches on the HIP stream
        sums.append(second[3])
    assert sums[0] == sums[1]


def test_direct_queue_interleaved_with_other_entry_points():
    """Every entry point other than the step calls uses the HIP stream and must first drain the library's own queue (check_handle ->
    leave_direct); the next step call waits for the stream and goes back to the queue.  A run chopped into many short calls with
    reads, writes and a second run in between must equal the same sequence on HIP-stream launches bit for bit."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, d = d100_gauss.Gauss_100D()._bpm_target_spec()
    N = 1024
    X0 = np.random.RandomState(9).normal(size=(N, d)) + 0.5
    outs = []
    for direct in (True, False):
        e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=21, burnin_gen=7, n_cr_gen=3)
        e.set_launch_path(direct)
        e.set_state(X0)
        e.begin_run()
        before = e.launch_stats()                                   # (the dispatch counters are per thread, not per sampler)
        seen = []
        for n in (0, 1, 2, 5, 1, 70, 3, 0, 64, 1):
            e.step(n)
            seen.append(e.get_state())                              # (drains the queue, reads through the stream)
            if n == 5:
                seen.append(e.get_loglike()[:8].copy())
                e.set_state(e.get_state() * 1.0)                    # a write through the stream between two direct-mode calls
            if n == 70:
                seen.append(np.asarray(e.stats()["p_cr"]))
                cnt, s1, s2, sh = e.reduce_moments(0)
                seen.append(np.concatenate([[cnt], s1, s2]))
        e.begin_run()                                               # a second run: counters reset, generation counter restarts
        e.step(9)
        ms, nl = e.step_timed(4)
        seen.append(e.get_history(0, e.history_rows()))
        seen.append(np.array([e.stats()["local_n_accepted"], e.stats()["k_gen"], e.history_rows()], dtype=float))
        ls = e.launch_stats()
        assert (ls["direct"] - before["direct"] > 0) == direct and (ls["stream"] - before["stream"] > 0) == (not direct)
        outs.append(seen)
        e.close()
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_two_samplers_of_one_thread_on_different_launch_paths_do_not_share_dispatch_state():
    """What the launch functions tell each other about where the current launches go is held per THREAD (sampler.hip: struct Dispatch), not per
    handle: two samplers alive in one thread, A on the library's own queue and B on HIP-stream launches, stepped alternately in short calls
    (across the end of burn-in, with a timed call of A between two calls of B), must each end exactly where the same sampler ends when it
    runs alone in the same call pattern -- state, ln-likes, history, p_cr bit for bit -- and every call's launches must be counted on the
    path of the sampler that made them."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, d = d100_gauss.Gauss_100D(dim=16)._bpm_target_spec()
    N, calls = 256, (1, 2, 5, 1, 20, 11)
    X0 = {"A": np.random.RandomState(3).normal(size=(N, d)) + 0.5, "B": np.random.RandomState(4).normal(size=(N, d)) - 0.5}

    def make(name):
        e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed={"A": 31, "B": 32}[name], burnin_gen=5, n_cr_gen=3)
        if name == "B":
            e.set_launch_path(False)
        e.set_state(X0[name])
        e.begin_run()
        return e

    def call(e, name, n, timed=False):          # one step call, its launches counted on the sampler's own path and on no other
        before = e.launch_stats()
        if timed:
            e.step_timed(n)
        else:
            e.step(n)
        after = e.launch_stats()
        mine, other = ("direct", "stream") if name == "A" else ("stream", "direct")
        assert after[mine] - before[mine] > 0 and after[other] == before[other], (name, n, before, after)

    def result(e):
        st = e.stats()
        return [e.get_state(), e.get_loglike(), e.get_history(0, e.history_rows()), np.asarray(st["p_cr"]), np.array([st["k_gen"], e.history_rows()], dtype=float)]

    def pattern(engines):                       # engines: {"A": ..., "B": ...} or one of the two alone
        for n in calls:
            for name in ("A", "B"):
                if name in engines:
                    call(engines[name], name, n)
            if n == 5 and "A" in engines:       # B's call of 5 generations before, B's call of 1 generation after
                call(engines["A"], "A", 3, timed=True)

    both = {"A": make("A"), "B": make("B")}
    pattern(both)
    together = {name: result(e) for name, e in both.items()}
    for e in both.values():
        e.close()
    for name in ("A", "B"):
        e = make(name)
        pattern({name: e})
        alone = result(e)
        e.close()
        assert alone[4][0] == sum(calls) + (3 if name == "A" else 0)
        for x, y in zip(together[name], alone):
            assert np.array_equal(x, y), name


@pytest.mark.parametrize("seq_seed", [77, 1234])
@pytest.mark.parametrize("case", ["dream_gauss100", "demc_banana_snooker", "dream_mix8"])
def test_random_call_sequences_equal_on_every_launch_path(case, seq_seed):
    """The steady state on the library's queue leaves the L2 write-back to the last dispatch of a step call (or to a fenced kernel at the
    drain) and sends what the next kernel reads through agent-scope stores: whatever a caller does between two step calls -- reads of
    state / ln-like / history rows / moments, writes of rows or of the whole state, launch-path switches, new runs -- must see and leave
    exactly what HIP-stream launches do.  Seeded random sequences of 150 such calls, three launch configurations, every read compared."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import banana_rv, d100_gauss, mixture_nd
    if case == "dream_gauss100":
        spec, algo, N, kw = d100_gauss.Gauss_100D()._bpm_target_spec(), L.ALGO_DREAM, 2048, dict(burnin_gen=9, n_cr_gen=3)
    elif case == "dream_mix8":
        spec, algo, N, kw = mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), L.ALGO_DREAM, 6000, dict(burnin_gen=12, n_cr_gen=3, outlier_every=5)
    else:
        spec, algo, N, kw = banana_rv.Banana_2D()._bpm_target_spec(), L.ALGO_DEMC, 3001, dict(p_snooker=0.15)
    tid, tp, d = spec
    X0 = np.random.RandomState(4).normal(size=(N, d)) + 0.7
    outs = []
    for direct, fence in ((True, -1), (False, -1), (True, 3)):
        rs = np.random.RandomState(seq_seed)                 # the same sequence for every configuration
        e = HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=31, **kw)
        e.set_launch_path(direct, fence)
        e.set_state(X0)
        e.begin_run()
        seen = []
        for _ in range(150):
            op = rs.randint(0, 10)
            if op <= 3:
                e.step(int(rs.choice([1, 1, 2, 3, 7, 20, 65])))
            elif op == 4:
                e.step_timed(int(rs.choice([1, 2, 9])))
            elif op == 5:
                seen.append(e.get_state())
            elif op == 6:
                seen.append(e.get_loglike().copy())
                rows = e.history_rows()
                lo = max(0, rows - 3)
                seen.append(e.get_history(lo, rows))
                seen.append(e.get_loglike_history(lo, rows))
            elif op == 7:
                X = e.get_state()
                X[rs.randint(0, N, size=5)] += 0.25                # rewrite a few rows through the stream
                e.set_state(X)
            elif op == 8:
                cnt, s1, s2, sh = e.reduce_moments(0)
                seen.append(np.concatenate([[cnt], s1, s2]))
                st = e.stats()
                seen.append(np.array([st["local_n_accepted"], st["local_n_rejected"], st["k_gen"]], dtype=float))
            else:
                flip = bool(rs.randint(0, 2))                                   # (drawn in every configuration)
                e.set_launch_path(direct and flip, fence)
        seen.append(e.get_state())
        seen.append(e.get_history(0, e.history_rows()))
        outs.append(seen)
        e.close()
    for o in outs[1:]:
        assert len(o) == len(outs[0])
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)


def test_sampler_sequence_in_one_process_keeps_histories_intact():
    """Samplers of different shapes created, run through both launch paths and destroyed one after the other in ONE process, then a
    run with a history row that is written twice (bpm_set_state in the middle) and a history that grows through several buffers: the
    four repetitions -- own queue, HIP stream, own queue, HIP stream -- must hold the same history bit for bit.  (With the state in
    the hardware-coherent memory type this is where rows came back with older contents: tools/coherent_memory_hazard.py.)"""
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(__file__), "..")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "coherent_memory_hazard.py")], cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "all four histories equal" in out.stdout, out.stdout[-2000:]


def test_running_moments_equal_history_moments_without_a_history():
    """param_est's mean / std (demc.py:242-246) for a burn-in of whole generations from per-generation population sums
    (bpm_config_t.running_moments): a sampler that keeps NO history must return what the history-based reduction returns, to 1e-12,
    on a 2000-generation run that passes through burn-in with CR adaptation and the outlier check (whose resets rewrite the last row)."""
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss, mixture_nd
    for spec, N, kw in ((d100_gauss.Gauss_100D()._bpm_target_spec(), 256, dict(burnin_gen=100, n_cr_gen=5)),
                        (mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), 512, dict(burnin_gen=300, n_cr_gen=5, outlier_every=50))):
        tid, tp, d = spec
        X0 = np.random.RandomState(4).normal(size=(N, d)) + 1.0
        G = 2000
        res = {}
        for label, keep, run in (("hist", True, False), ("sums", False, True), ("both", True, True)):
            if label == "sums" and "outlier_every" in kw:
                continue                      # (the outlier check itself needs the log-like history)
            e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=17, keep_history=keep,
                          running_moments=run, **kw)
            e.set_state(X0)
            e.begin_run()
            e.step(700)
            e.step(G - 700)
            out = {}
            for n_burn in (0, N * 1, N * 401, N * 1999, N * (G + 1)):
                cnt, s1, s2, sh = e.reduce_moments(n_burn)
                out[n_burn] = (cnt, sh + s1 / max(cnt, 1), np.sqrt(np.maximum(s2 / max(cnt, 1) - (s1 / max(cnt, 1)) ** 2, 0.0)))
            if label == "sums":
                with pytest.raises(L.BpmError, match="multiple of n_chains"):
                    e.reduce_moments(N * 3 + 1)
                assert e.history_rows() <= 1
            res[label] = (out, e.get_state())
            e.close()
        for label in res:
            assert np.array_equal(res[label][1], res["hist"][1])                  # the same run
            for n_burn, (cnt, mean, std) in res[label][0].items():
                c0, m0, s0 = res["hist"][0][n_burn]
                assert cnt == c0
                if cnt:
                    np.testing.assert_allclose(mean, m0, rtol=1e-12, atol=1e-12)
                    np.testing.assert_allclose(std, s0, rtol=1e-10, atol=1e-12)


def test_sampler_class_without_history_still_estimates_parameters():
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.5, dim=10)
    a = DreamMpi(t.ln_like, np.zeros(10), n_chains=64, n_cr_gen=3, burnin_gen=10, seed=5)
    b = DreamMpi(t.ln_like, np.zeros(10), n_chains=64, n_cr_gen=3, burnin_gen=10, seed=5, keep_history=False)
    a.run_mcmc(64 * 300)
    b.run_mcmc(64 * 300)
    ma, sa = a.param_est_moments(64 * 100)
    mb, sb = b.param_est_moments(64 * 100)
    mean, std, _ = a.param_est(64 * 100)
    np.testing.assert_allclose(mb, ma, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(sb, sa, rtol=1e-10)
    np.testing.assert_allclose(mb, mean, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(sb, std, rtol=1e-9)


def test_drains_at_every_position_of_the_queues_epochs():
    """The library's own AQL queue closes every epoch of 256 packets with a marker packet of its own, and a drain behind release-less packets of
    a SMALL population (fewer than 64 workgroups: the last update kernel's release is not a full write-back) dispatches an empty fence kernel before its
    barrier packet.  When that kernel took position 254 of an epoch IN THE RING'S FIRST LAP the marker behind it stayed unpublished while the
    barrier packet's doorbell was rung: the packet processor stopped in front of an INVALID header and the drain ran into its time limit (found
    when a longer test file shifted the suite's packet count onto that position).  Here: in a fresh process the queue is padded so that the drain's
    packets sit just in front of the marker in every epoch of the first two laps (fence kernel at 254 in the first), then drains at random positions.
    In a child process: the time limit is read once per process, and the first lap exists once."""
    import subprocess
    code = r'''
import ctypes as C, os, sys, numpy as np
sys.path.insert(0, os.getcwd())
from bipymc_amd import _lib as L
from bipymc_amd.engine import HipEngine
from bipymc_amd.utils import d100_gauss
tid, tp, d = d100_gauss.Gauss_100D(dim=8)._bpm_target_spec()
e = HipEngine(algo=L.ALGO_DREAM, n_chains=20, dim=d, target_id=tid, target_params=tp, seed=3, burnin_gen=0, keep_history=False)
e.set_state(np.random.RandomState(0).normal(size=(20, d)))
e.begin_run()
ls0 = e.launch_stats()
assert ls0["has_queue"], ls0
e.step(1)
e.synchronize()                                   # (the first table build is behind us)
w = C.c_int64(0)
n = 1
for epoch, start in enumerate((252, 251, 252, 250, 252, 253, 254, 252)):   # 2 update packets, then the drain's fence kernel + barrier packet: fence at start + 2
    L.check(e.lib.bpm_debug_queue_pad(e._h, start, C.byref(w)), e.lib)
    assert w.value == 256 * epoch + start, (w.value, epoch, start)           # epochs 0 ... 3 are the ring's first lap
    e.step(1)
    e.synchronize()
    n += 1
    print("drain behind position", start, "ok", flush=True)
rs = np.random.RandomState(1)
for i in range(400):
    k = int(rs.randint(1, 4))
    e.step(k)
    e.synchronize()
    n += k
ls = e.launch_stats()
assert ls["direct"] - ls0["direct"] == 2 * n and ls["stream"] == ls0["stream"], (ls0, ls)
print("DRAINS-OK", n)
'''
    env = dict(os.environ, BPM_QUEUE_TIMEOUT_S="15", BPM_LIB_PATH=_test_lib_path())       # (bpm_debug_queue_pad: a hook of the test variant)
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DRAINS-OK" in out.stdout, out.stdout[-1500:] + out.stderr[-2500:]
