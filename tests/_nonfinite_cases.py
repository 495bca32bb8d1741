"""Shared pieces of tests/test_gpu_nonfinite.py and tests/test_nonfinite_host.py: ln-likelihoods that return -inf, NaN and +inf, in every form the
sampler accepts, the start states that put chains outside the support, and the oracle's run of every case (computed once per process, never changed).

The Metropolis step under test is samplers.py:328-336 as oracle/sampler_ref.py restates it (mut_prop_ratio / metropolis_accept):
    alpha = clip(min(1, exp(ll_prop - ll_cur)), 0, 1);  accepted = u < alpha
  ll_prop = -inf, ll_cur finite     -> alpha = 0: never accepted
  ll_cur  = -inf, ll_prop finite    -> alpha = +inf clipped to 1: always accepted
  both -inf, both +inf, either NaN  -> alpha = NaN: never accepted, counted (n_nan / stats()["n_nan_alpha"])
  ll_prop = +inf, ll_cur finite     -> alpha = 1: always accepted; the chain then stays (alpha = 0 or NaN from there)
"""
import functools

import numpy as np

from oracle import sampler_ref as R

RHO = 0.4
MARGIN = 1e-6          # oracle and kernel agree on a proposal to ~1e-11 relative: no proposal may lie closer than this to a face of the box (or of a band)
GENS = 9


def sigma_of(d):
    return np.sqrt(np.arange(d) + 1.0)


def bound_of(d):
    return 2.5 if d <= 10 else (3.5 if d <= 100 else 4.0)


def box_params(d):
    """[rho, c0, a, b, 1/sigma_0 .. 1/sigma_{d-1}] of R.gauss_equicorr_params, then [bound, lower band edge, upper band edge]"""
    s = sigma_of(d)
    return np.concatenate([R.gauss_equicorr_params(RHO, s), [bound_of(d), -2.0, 2.0 * s[0]]])


class BoxLikelihood(object):
    """The equicorrelated Gaussian (rho = 0.4, sigma_j = sqrt(j + 1)) truncated to the box |x_j| / sigma_j <= bound: -inf outside.
    variant "bands": inside the box NaN where x_0 < -2 and +inf where x_0 > 2 sigma_0.  The callable records the smallest distance of any row it has
    evaluated from a face of the box (in units of sigma_j) and, for "bands", of x_0 from a band edge."""

    def __init__(self, d, variant):
        assert variant in ("box", "bands")
        self.d, self.variant = int(d), variant
        self.params = box_params(d)
        self.isig = self.params[4:4 + d]
        self.bound, self.lo_band, self.hi_band = self.params[4 + d:]
        self.margin = np.inf
        self.n_returned = dict(nan=0, pinf=0, minf=0, finite=0)      # how often each value class came back

    def __call__(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        v = self._value(theta)
        self.n_returned["nan" if v != v else "pinf" if v == np.inf else "minf" if v == -np.inf else "finite"] += 1
        return v

    def _value(self, theta):
        z = theta * self.isig
        self.margin = min(self.margin, float(np.min(np.abs(np.abs(z) - self.bound))))
        if np.any(np.abs(z) > self.bound):
            return -np.inf
        if self.variant == "bands":
            self.margin = min(self.margin, abs(theta[0] - self.lo_band), abs(theta[0] - self.hi_band))
            if theta[0] < self.lo_band:
                return np.nan
            if theta[0] > self.hi_band:
                return np.inf
        return float(R.ll_gauss_equicorr(theta, self.params[:4 + self.d]))

    def rows(self, X):
        return np.array([self(x) for x in X], dtype=np.float64)


_HIP_BANDS = """
    const double x0 = X0_EXPR;
    if (x0 < p[5 + d]) return __builtin_nan("");
    if (x0 > p[6 + d]) return __builtin_inf();"""


def hip_source(variant, terms):
    """-> (source, terms) for HipEngine.set_device_likelihood / HipLikelihood: the whole-row form (terms = 0) or the per-coordinate form, whose third
    accumulator counts the coordinates outside the box ("bands": a fourth carries x_0 to ln_like_finish)."""
    bands = _HIP_BANDS if variant == "bands" else ""
    if not terms:
        return """
__device__ double ln_like(const double* x, int d, const double* p) {      // p = [rho, c0, a, b, 1/sigma ..., bound, lower band edge, upper band edge]
    double s1 = 0.0, s2 = 0.0;
    int n_out = 0;
    for (int j = 0; j < d; ++j) { const double z = x[j] * p[4 + j]; s1 += z; s2 += z * z; n_out += (fabs(z) > p[4 + d]) ? 1 : 0; }
    if (n_out != 0) return -__builtin_inf();%s
    return p[1] - 0.5 * (p[2] * s2 - p[3] * s1 * s1);
}
""" % bands.replace("X0_EXPR", "x[0]"), 0
    k = 4 if variant == "bands" else 3
    return """
#define BPM_LN_LIKE_TERMS %d
__device__ void ln_like_terms(double xj, int j, int d, const double* p, double* acc) {
    const double z = xj * p[4 + j];
    acc[0] += z; acc[1] += z * z; acc[2] += (fabs(z) > p[4 + d]) ? 1.0 : 0.0;%s
}
__device__ double ln_like_finish(const double* acc, int d, const double* p) {
    if (acc[2] != 0.0) return -__builtin_inf();%s
    return p[1] - 0.5 * (p[2] * acc[1] - p[3] * acc[0] * acc[0]);
}
""" % (k, "\n    if (j == 0) acc[3] += xj;" if variant == "bands" else "", bands.replace("X0_EXPR", "acc[3]")), k


def torch_ll_factory(torch, d, variant):
    """the same function on device tensors, built the way tests/_torch_worker.py builds its Gaussian: rows -> (n,) float64 on the device"""
    tp = torch.tensor(box_params(d), dtype=torch.float64, device="cuda")

    def torch_ll(rows):
        X = torch.as_tensor(rows, device="cuda")
        z = X * tp[4:4 + d]
        s1, s2 = z.sum(dim=1), (z * z).sum(dim=1)
        val = tp[1] - 0.5 * (tp[2] * s2 - tp[3] * s1 * s1)
        if variant == "bands":
            val = torch.where(X[:, 0] < tp[5 + d], torch.full_like(val, float("nan")), val)
            val = torch.where(X[:, 0] > tp[6 + d], torch.full_like(val, float("inf")), val)
        return torch.where((z.abs() > tp[4 + d]).any(dim=1), torch.full_like(val, float("-inf")), val)

    return torch_ll


def start_state(k, N, d, every=4):
    """RandomState(k).normal * sigma with every `every`-th row multiplied by 3: those chains start outside the box"""
    X = np.random.RandomState(k).normal(size=(N, d)) * sigma_of(d)
    X[::every] *= 3.0
    return X


# ---- section 1: (name, algo, d, N, sampler keywords, every n-th start row outside, start seed, oracle seed) ----------------------------------------
# the shapes of tests/test_gpu_parity.py's propose / commit and HIP-source drivers that reach each kernel: 4 lanes / 16 lanes / one wavefront per chain,
# the looped wide-row kernel and its commit kernel (d = 600, d = 1201: odd), the outlier check with chains at -inf (N = 40: they are the ones reset;
# N = 700: the quartiles are not finite and nobody is), DE-MC with snooker, synchronous DE-MC's x_next branch.  The start seed of each case is the first
# (from 5 up) under which the oracle's run of BOTH variants meets every precondition tests/test_nonfinite_host.py asserts: at d >= 150 a chain comes back
# into the box only from a row that is outside by one coordinate, which few starts of ten or twelve chains hold.
BOX_CASES = [
    ("dream-d10-N16", R.ALGO_DREAM, 10, 16, dict(burnin_gen=6, n_cr_gen=2), 4, 8, 78),
    ("dream-d100-N64", R.ALGO_DREAM, 100, 64, dict(burnin_gen=5, n_cr_gen=1), 4, 5, 78),
    ("dream-d600-N12", R.ALGO_DREAM, 600, 12, dict(burnin_gen=5, n_cr_gen=1), 4, 77, 78),
    ("dream-d1201-N10", R.ALGO_DREAM, 1201, 10, dict(burnin_gen=4, n_cr_gen=1), 4, 34, 78),
    ("dream-d8-N40-outlier", R.ALGO_DREAM, 8, 40, dict(burnin_gen=6, n_cr_gen=1, outlier_every=2), 13, 6, 78),
    ("dream-d8-N700-outlier", R.ALGO_DREAM, 8, 700, dict(burnin_gen=6, n_cr_gen=1, outlier_every=2), 4, 5, 78),
    ("demc-d2-N24", R.ALGO_DEMC, 2, 24, dict(p_snooker=0.3), 4, 5, 78),
    ("demc-d150-N40", R.ALGO_DEMC, 150, 40, dict(p_snooker=0.2), 4, 16, 78),
    ("sync-d3-N10", R.ALGO_DEMC_SYNC, 3, 10, dict(), 4, 6, 78),
    ("sync-d100-N24", R.ALGO_DEMC_SYNC, 100, 24, dict(), 4, 7, 78),
    ("sync-d600-N12", R.ALGO_DEMC_SYNC, 600, 12, dict(), 4, 77, 78),
]
BOX_BY_NAME = {c[0]: c for c in BOX_CASES}
VARIANTS = ("box", "bands")
# the propose / commit path has no outlier check (the host drives it generation by generation)
COMMIT_CASES = [c[0] for c in BOX_CASES if "outlier_every" not in c[4]]
# the device-resident driver's own three shapes (tests/test_gpu_parity.py::test_device_resident_likelihood_against_oracle)
DEVICE_CASES = [
    ("dream-d10-N24", R.ALGO_DREAM, 10, 24, dict(del_pairs=3, burnin_gen=5, n_cr_gen=2), 4, 6, 79),
    ("dream-d101-N40", R.ALGO_DREAM, 101, 40, dict(del_pairs=3, burnin_gen=4, n_cr_gen=2), 4, 8, 79),
    ("demc-d4-N30", R.ALGO_DEMC, 4, 30, dict(p_snooker=0.2), 4, 5, 79),
]
BOX_BY_NAME.update({c[0]: c for c in DEVICE_CASES})


def value_classes(a):
    """(NaN mask, +inf mask, -inf mask) of an array"""
    a = np.asarray(a)
    return np.isnan(a), a == np.inf, a == -np.inf


def assert_same_classes_and_close(got, want, rtol, atol, what=""):
    """non-finite values in the same class at the same positions (each class on its own), then the finite rest within the tolerance"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for name, g, w in zip(("NaN", "+inf", "-inf"), value_classes(got), value_classes(want)):
        assert np.array_equal(g, w), "%s: %s at other positions: kernel %s, oracle %s" % (what, name, np.argwhere(g)[:8].tolist(), np.argwhere(w)[:8].tolist())
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


class OracleRun(object):
    """What the oracle did in one case, generation by generation (index g = state AFTER generation g - 1; 0 = the start)."""


@functools.lru_cache(maxsize=None)
def oracle_box_run(name, variant):
    _n, algo, d, N, kw, every, k_start, seed = BOX_BY_NAME[name]
    ll = BoxLikelihood(d, variant)
    ora = R.OracleSampler(algo, N, d, R.TARGET_HOST, None, seed, ll_fn=ll, **kw)
    X0 = start_state(k_start, N, d, every)
    ora.set_state(X0)
    ll.margin = np.inf                                  # (the start rows are set by the test, not proposed: tripled rows lie wherever they lie)
    r = OracleRun()
    r.name, r.variant, r.algo, r.d, r.N, r.kw, r.seed, r.X0 = name, variant, algo, d, N, dict(kw), seed, X0
    r.ll0 = ora.ll.copy()
    r.X, r.ll, r.acc, r.from_minf, r.n_acc, r.n_rej, r.n_nan, r.p_cr, r.resets = [X0.copy()], [ora.ll.copy()], [], [], [], [], [], [], []
    for g in range(GENS):
        ora.trace = []
        ll_before = ora.ll.copy()
        with np.errstate(invalid="ignore"):             # (the outlier check's quartiles of mean ln-likes that hold -inf)
            ora._generation(g, 0.5, True, 1e-12 if algo == R.ALGO_DREAM else 1e-15, 1e-2, None)
        tr = ora.trace[0]
        acc = np.zeros(N, dtype=bool)
        if algo == R.ALGO_DEMC_SYNC:
            acc[:] = tr["accepted"]
        else:
            for ph in ("phase0", "phase1"):
                acc[tr[ph]["ids"]] = tr[ph]["accepted"]
        r.acc.append(acc)
        r.from_minf.append(acc & (ll_before == -np.inf))            # ll_cur = -inf, the proposal inside the box: always accepted, the chain moves
        r.X.append(ora.X.copy())
        r.ll.append(ora.ll.copy())
        r.n_acc.append(ora.local_n_accepted)
        r.n_rej.append(ora.local_n_rejected)
        r.n_nan.append(ora.n_nan)
        r.p_cr.append(ora.cr.p_cr.copy())
        r.resets.append(ora.n_outlier_resets)
    r.history = ora.history_array()
    r.ll_history = np.stack(ora.ll_history, axis=0)
    r.n_cr_updates = ora.cr.n_cr_updates.copy()
    r.margin = ll.margin
    r.n_returned = dict(ll.n_returned)
    for a in (r.history, r.ll_history, r.X0, r.ll0):
        a.setflags(write=False)
    return r


# ---- section 2: the shipped targets from overflow start rows -----------------------------------------------------------------------------------------
# A row of magnitude 1e160 overflows z * z: the Gaussian and the mixture give NaN, the banana -inf; gamma (a - b) stays finite, so a chain that draws
# such a row as a partner proposes at that scale and is rejected.  DREAM runs with burnin_gen = 0 here: from these starts the oracle's own p_cr becomes
# NaN (delta_m sums a NaN jump distance), so with CR adaptation the reference defines nothing to compare with; section 1 covers adaptation.
OVERFLOW_GENS = 8
OVERFLOW_CASES = (
    [("dream", "gauss", sh, pairs) for pairs in (3, 2) for sh in range(7)] +
    [("dream", "mix", sh, pairs) for pairs in (3, 2) for sh in (1, 3, 6)] +
    [("dream", "banana", 0, pairs) for pairs in (3, 2)] +
    [("demc", "gauss", sh, 1) for sh in (0, 3, 5, 6)] + [("demc", "mix", 1, 1), ("demc", "banana", 0, 1)] +
    [("sync", "gauss", sh, 1) for sh in (0, 3, 6)] + [("sync", "banana", 0, 1)])
OVERFLOW_IDS = ["%s-%s-shape%d-pairs%d" % c for c in OVERFLOW_CASES]


def overflow_rows(X0):
    """row 1 = 1e160 * (+1, -1, +1, ...), row 5 = 1e160"""
    X0 = np.array(X0, dtype=np.float64, copy=True)
    d = X0.shape[1]
    X0[1] = 1e160 * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    X0[5] = 1e160
    return X0


def overflow_case(algo_name, kind, shape, pairs):
    """-> (algo, N, d, target id, parameter block, seed, start state, sampler keywords, launches): the kernel shapes' widths and the targets' start
    states are tests/test_gpu_shipped_path.py's own (_SHAPE_DIMS, _target_case), the sizes its table test's (N = 96 / 40 for DREAM, 130 / 48 for DE-MC)"""
    from test_gpu_shipped_path import _SHAPE_DIMS, _target_case as target_case      # (here: that module imports this one)
    d = 2 if kind == "banana" else _SHAPE_DIMS[shape]
    v = {"demc": 0, "sync": 0}.get(algo_name, 1 if pairs == 3 else 2)
    rs = np.random.RandomState(100 * v + shape + (0 if kind == "gauss" else 50 if kind == "mix" else 90))
    if algo_name == "dream":
        algo, N, kw = R.ALGO_DREAM, (40 if d > 128 else 96), dict(del_pairs=pairs, n_cr=3, burnin_gen=0)
    elif algo_name == "demc":
        algo, N, kw = R.ALGO_DEMC, (48 if d > 128 else 130), dict(p_snooker=0.2)
    else:
        algo, N, kw = R.ALGO_DEMC_SYNC, (48 if d > 128 else 130), dict()
    tid, params, X0 = target_case(kind, N, d, rs)
    launches = (0, OVERFLOW_GENS) if algo_name == "sync" else None
    return algo, N, d, tid, params, 300 + 10 * v + shape, overflow_rows(X0), kw, launches
