"""bipymc_amd/traces.py without a GPU: traces.compute driven by a NumPy stand-in for the two device calls (the same bins, shifts and shifted
sums as bipymc_amd/csrc/traces.h hands over, added as blocked partials in another order than NumPy's), on 1, 2 and 4 emulated ranks.

Tolerance (derived, not measured).  u = 2^-53.  A bin of n finite values has exact mean m, variance var and D = max |x - m|.  A rank sums
d = x - c with the shift c one of the bin's values, so |c - m| <= D, |d| <= 2 D and sum d^2 / n = var + (c - m)^2 <= 2 D^2.
  d itself carries one rounding, |fl(d) - d| <= u |d|.  Summing n terms in any order has error <= gamma_n sum |terms|, gamma_n ~ n u (Higham,
  Accuracy and Stability of Numerical Algorithms, section 4.2), so S1 / n is off by <= (n + 1) u 2 D and S2 / n by <= (n + 3) u 2 D^2.
  mean = c + S1 / n adds two roundings of values <= max |x| + 2 D <= 3 max |x|, and D <= 2 max |x|:
      |mean - m| <= (4 (n + 1) + 6) u max |x| <= 8 (n + 8) u max |x|.
  sd^2 = S2 / n - (S1 / n)^2 with |S1 / n| = |m - c| <= D: the second term is off by <= 2 D (n + 1) u 2 D + O(u D^2), the whole by
      |sd^2 - var| <= ((2 n + 6) + (4 n + 8)) u D^2 <= 8 (n + 8) u D^2,
  which leaves 2 n u D^2 for the rank merge and the square root.  The merge is Chan's formula on R parts with the running mean carried
  as shift + offset (traces.merge_moments): delta = (c_r - c) + (off_r - off) is a difference of numbers <= 2 D with O(u D) error, so
  delta^2 n_a n_b / n adds O(u n D^2) before the division by n.  (Formed from the rounded means, delta would be off by u |mean| and
  sd^2 by 2 D u |mean|: at an offset of 1e8 that is 1e8 / D times the bound -- the first version of this merge failed this test so.)
  Merging two accumulators of different shifts (traces.h: tr_merge_moments) rewrites B's sums about A's shift, a few roundings of
  values <= 4 n_B D^2: O(u D^2) after the division by n, inside the same room.
The model assumes no underflow.  IEEE gradual underflow adds an ABSOLUTE error of at most 2^-1075 per operation whose result is subnormal
(the products d^2 and the divisions; sums of subnormals are exact); after the division by n that is at most one unit 2^-1074 per formula
line above, so the bounds carry + 2 * 2^-1074 (mean) and + 4 * 2^-1074 (sd^2).  They matter for a column of denormals only.
The comparison value is computed in np.longdouble (or math.fsum) from the history itself.  Everything else -- min, max, counts, best_*,
chain_*, gen, n -- is compared for equality."""
import math
import warnings

import numpy as np
import pytest

from bipymc_amd import traces as TR

U = 2.0 ** -53
TINY = 2.0 ** -1074


def trace_bound(n, max_abs, D):
    """-> (bound on |mean - m|, bound on |sd^2 - var|) for a bin of n finite values, max_abs = max |x|, D = max |x - m| (module docstring)"""
    k = 8.0 * (n + 8) * U
    return k * max_abs + 2 * TINY, k * D * D + 4 * TINY


def _check_moments(mean, sd, X, what):
    """mean, sd of the device against the columns of X (rows, cols): NumPy's answer where it is not finite, the bound where it is"""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_m, want_s = np.mean(X, axis=0), np.std(X, axis=0)
    fin = np.isfinite(X).all(axis=0)
    assert np.array_equal(mean[~fin], want_m[~fin], equal_nan=True), what
    assert np.all(np.isnan(sd[~fin])) and np.all(np.isnan(want_s[~fin])), what
    for k in np.nonzero(fin)[0]:
        x = X[:, k].astype(np.longdouble)
        m = x.sum() / len(x)
        var = ((x - m) ** 2).sum() / len(x)
        bm, bv = trace_bound(len(x), float(np.abs(X[:, k]).max()), float(np.abs(x - m).max()))
        assert abs(np.longdouble(mean[k]) - m) <= bm, (what, k, float(abs(np.longdouble(mean[k]) - m)), bm)
        assert abs(np.longdouble(sd[k]) ** 2 - var) <= bv, (what, k, float(abs(np.longdouble(sd[k]) ** 2 - var)), bv)


def check_against_numpy(pt, H, LL, n_burn, every, chains=None):
    """pt: the PosteriorTrace of the history H (G, N, d) with log-likelihoods LL (G, N) -- every field against NumPy on these arrays"""
    H, LL = np.asarray(H), np.asarray(LL)
    G, N, d = H.shape
    g0 = -(-n_burn // N)
    ev = min(every, G - g0)
    gen = np.arange(g0, G, ev)
    T = len(gen)
    assert pt.gen.dtype == np.int64 and np.array_equal(pt.gen, gen)
    assert pt.n.dtype == np.int64 and np.array_equal(pt.n, (np.minimum(gen + ev, G) - gen) * N)
    assert pt.mean.shape == pt.sd.shape == pt.min.shape == pt.max.shape == pt.n_nan.shape == (T, d)
    assert pt.ll_mean.shape == pt.ll_min.shape == pt.ll_max.shape == (T,) and pt.n_nan.dtype == np.int64
    for t, ga in enumerate(gen):
        W = H[ga:min(ga + ev, G)].reshape(-1, d)
        L = LL[ga:min(ga + ev, G)].reshape(-1, 1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert np.array_equal(pt.min[t], np.nanmin(W, axis=0), equal_nan=True), t
            assert np.array_equal(pt.max[t], np.nanmax(W, axis=0), equal_nan=True), t
            assert np.array_equal([pt.ll_min[t]], np.nanmin(L, axis=0), equal_nan=True), t
            assert np.array_equal([pt.ll_max[t]], np.nanmax(L, axis=0), equal_nan=True), t
        assert np.array_equal(pt.n_nan[t], np.isnan(W).sum(axis=0)), t
        _check_moments(pt.mean[t], pt.sd[t], W, ("bin", t))
        _check_moments(pt.ll_mean[t:t + 1], np.full(1, np.nan) if not np.isfinite(L).all() else _ll_sd(L), L, ("ln-like of bin", t))
    flat = LL[g0:].reshape(-1)
    if np.all(np.isnan(flat)):
        assert pt.best_row == -1 and np.isnan(pt.best_ll) and np.all(np.isnan(pt.best_x))
    else:
        row = g0 * N + int(np.nanargmax(flat))
        assert pt.best_row == row and pt.best_ll == LL.reshape(-1)[row]
        assert np.array_equal(pt.best_x.view(np.uint64), H.reshape(-1, d)[row].view(np.uint64))
    ch = np.zeros(0, dtype=np.int64) if chains is None else np.asarray(chains, dtype=np.int64)
    assert np.array_equal(pt.chains, ch)
    assert pt.chain_x.shape == (T, len(ch), d) and pt.chain_ll.shape == (T, len(ch))
    assert np.array_equal(pt.chain_x.view(np.uint64), np.ascontiguousarray(H[gen][:, ch]).view(np.uint64))
    assert np.array_equal(pt.chain_ll.view(np.uint64), np.ascontiguousarray(LL[gen][:, ch]).view(np.uint64))
    lo, hi = pt.band(2.0)
    assert np.array_equal(lo, pt.mean - 2.0 * pt.sd, equal_nan=True) and np.array_equal(hi, pt.mean + 2.0 * pt.sd, equal_nan=True)


def _ll_sd(L):
    """(PosteriorTrace has no ll_sd: the exact one stands in, so that _check_moments checks ll_mean alone)"""
    x = L[:, 0].astype(np.longdouble)
    return np.array([float(np.sqrt(((x - x.sum() / len(x)) ** 2).sum() / len(x)))])


class FakeRanks(object):
    """The device calls of R ranks over the history H (G, N, d) and its log-likelihoods LL (G, N): rank r holds the chains [r N / R,
    (r + 1) N / R).  What traces.h hands over, restated: the shift is the rank's first finite value of the bin, the sums are 7 blocked
    partials added last to first."""

    def __init__(self, H, LL, R):
        self.H, self.LL, self.R = np.asarray(H, dtype=np.float64), np.asarray(LL, dtype=np.float64), R
        self.G, self.N, self.d = self.H.shape
        self.n_local = self.N // R
        self.calls = []

    @staticmethod
    def _column(x):
        """-> (n, n_nan, n_pinf, n_ninf), (c, S1, S2, min, max) of a 1-D array"""
        fin = x[np.isfinite(x)]
        c = fin[0] if len(fin) else 0.0
        s1 = s2 = 0.0
        for b in reversed(np.array_split(fin - c, 7)):
            s1 += float(b.sum())
            s2 += float((b * b).sum())
        ok = x[~np.isnan(x)]
        return ((len(fin), int(np.isnan(x).sum()), int((x == np.inf).sum()), int((x == -np.inf).sum())),
                (c, s1, s2, ok.min() if len(ok) else np.inf, ok.max() if len(ok) else -np.inf))

    def trace_bins(self, g0, g1, every):
        gen = np.arange(g0, g1, every)
        T, d = len(gen), self.d
        self.gen = gen
        out = []
        for r in range(self.R):
            sl = slice(r * self.n_local, (r + 1) * self.n_local)
            counts, sums = np.zeros((2, T, d), dtype=np.int64), np.zeros((5, T, d))
            llc, lls = np.zeros((4, T), dtype=np.int64), np.zeros((5, T))
            for t, ga in enumerate(gen):
                W = self.H[ga:min(ga + every, g1), sl].reshape(-1, d)
                for k in range(d):
                    cnt, sm = self._column(W[:, k])
                    counts[:, t, k], sums[:, t, k] = cnt[:2], sm
                llc[:, t], lls[:, t] = self._column(self.LL[ga:min(ga + every, g1), sl].reshape(-1))
            L = self.LL[g0:g1, sl]
            if np.all(np.isnan(L)):
                best = (np.nan, -1, np.full(d, np.nan))
            else:
                g, i = np.unravel_index(np.nanargmax(L), L.shape)
                best = (L[g, i], (g0 + g) * self.N + r * self.n_local + i, self.H[g0 + g, r * self.n_local + i].copy())
            out.append((counts, sums, llc, lls) + best)
        return out

    def trace_chains(self, chains):
        ch = np.asarray(chains)
        self.calls.append(ch.copy())
        out = []
        for r in range(self.R):
            pos = np.nonzero((ch >= r * self.n_local) & (ch < (r + 1) * self.n_local))[0]
            out.append((pos, self.H[self.gen][:, ch[pos]], self.LL[self.gen][:, ch[pos]]))
        return out


def _compute(fr, n_burn=0, every=1, chains=None):
    return TR.compute(fr.trace_bins, fr.trace_chains, lambda x: x, n_burn, fr.N, fr.G, fr.d, every=every, chains=chains)


def _history(G=23, N=16, d=5, seed=3):
    rs = np.random.RandomState(seed)
    H = rs.normal(size=(G, N, d))
    H[:, :, 1] = 1e8 + H[:, :, 1]                 # far from the origin, unit spread
    H[:, :, 2] = -0.25                            # constant
    H[:, :, 3] = rs.randint(0, 50, size=(G, N)) * 5e-324
    LL = -0.5 * (H[:, :, 0] ** 2 + H[:, :, 4] ** 2) - 1e5
    return H, LL


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("every,n_burn", [(1, 0), (4, 0), (5, 16 * 2 + 1), (23, 0), (1000, 7)])
def test_rank_merge_equals_the_pooled_answer_and_ragged_last_bin(R, every, n_burn):
    H, LL = _history()
    pt = _compute(FakeRanks(H, LL, R), n_burn, every, chains=[15, 0, 9])
    check_against_numpy(pt, H, LL, n_burn, every, chains=[15, 0, 9])
    assert np.all(pt.sd[:, 2] == 0.0) and np.all(pt.mean[:, 2] == -0.25)
    if (every, n_burn) == (5, 33):
        assert pt.gen.tolist() == [3, 8, 13, 18] and pt.n.tolist() == [80, 80, 80, 80]      # g0 = ceil(33 / 16); 23 - 3 = 4 x 5
    if (every, n_burn) == (4, 0):
        assert pt.gen.tolist() == [0, 4, 8, 12, 16, 20] and pt.n[-1] == 3 * 16              # the last bin is short
    if every >= 23:
        assert len(pt.gen) == 1 and pt.n[0] == (23 - pt.gen[0]) * 16


def test_values_that_are_not_finite_follow_numpy():
    H, LL = _history(G=12)
    H[2, 3, 0] = np.nan
    H[3, :, 0] = np.nan                           # every value of a bin
    H[5, 1, 0] = np.inf
    H[6, 2, 0] = -np.inf
    H[7, 1, 0], H[7, 9, 0] = np.inf, -np.inf
    H[8, 0, 1] = np.nan                           # the rank's first row of the bin: the shift must be another value
    H[9, :9, 1] = np.inf                          # ... and a whole rank's first rows
    for R in (1, 2, 4):
        for every in (1, 2, 12):
            check_against_numpy(_compute(FakeRanks(H, LL, R), 0, every), H, LL, 0, every)
    pt = _compute(FakeRanks(H, LL, 2))
    assert np.isnan(pt.min[3, 0]) and np.isnan(pt.max[3, 0]) and pt.n_nan[3, 0] == 16 and pt.n_nan[2, 0] == 1
    assert pt.mean[5, 0] == np.inf and pt.mean[6, 0] == -np.inf and np.isnan(pt.mean[7, 0]) and np.isnan(pt.sd[5, 0])
    assert pt.min[6, 0] == -np.inf and pt.max[5, 0] == np.inf


@pytest.mark.parametrize("values,want", [
    ([1.0, 2.0, 3.0, 6.0], 3.0), ([1.0, np.nan, 3.0, 6.0], np.nan), ([1.0, np.inf, 3.0, 6.0], np.inf), ([-np.inf, 2.0, 3.0, -np.inf], -np.inf),
    ([np.inf, 2.0, -np.inf, 6.0], np.nan), ([np.inf, np.nan, 3.0, 6.0], np.nan), ([np.nan] * 4, np.nan), ([-np.inf] * 4, -np.inf),
    ([np.inf, np.inf, np.inf, -np.inf], np.nan)])
def test_ll_mean_table(values, want):
    H, LL = _history(G=3, N=4)
    LL[1] = values
    for R in (1, 2):
        pt = _compute(FakeRanks(H, LL, R))
        with np.errstate(invalid="ignore"):
            assert np.array_equal([pt.ll_mean[1]], [np.mean(values)], equal_nan=True)
        assert np.array_equal([pt.ll_mean[1]], [want], equal_nan=True)
        ok = [v for v in values if v == v]
        assert np.array_equal([pt.ll_min[1], pt.ll_max[1]], [min(ok), max(ok)] if ok else [np.nan, np.nan], equal_nan=True)
        check_against_numpy(pt, H, LL, 0, 1)


def test_best_row_ties_and_nan():
    H, LL = _history(G=6, N=8)
    LL[:] = -5.0
    LL[2, 6] = LL[2, 1] = LL[4, 0] = 7.5          # a tie inside a generation across ranks, and a later generation
    LL[1, 3] = np.nan
    for R in (1, 2, 4):
        pt = _compute(FakeRanks(H, LL, R))
        assert pt.best_row == 2 * 8 + 1 and pt.best_ll == 7.5 and np.array_equal(pt.best_x, H[2, 1])
        pt = _compute(FakeRanks(H, LL, R), n_burn=2 * 8 + 2, every=2)         # the window starts at generation 3
        assert pt.best_row == 4 * 8 and np.array_equal(pt.best_x, H[4, 0])
    best = TR.pick_best([(1.0, 9, [0.0]), (1.0, 4, [1.0]), (1.0, 4, [2.0]), (np.nan, 0, [3.0]), (2.0, -1, [4.0])])
    assert best[:2] == (1.0, 4) and best[2].tolist() == [1.0]                     # equal rows: the first rank
    assert TR.pick_best([(0.0, 9, [0.0]), (-0.0, 4, [1.0])])[1] == 4              # -0.0 == 0.0: the smaller row
    LL[:] = -np.inf
    pt = _compute(FakeRanks(H, LL, 2))
    assert pt.best_row == 0 and pt.best_ll == -np.inf                             # -inf is a log-likelihood like any other
    LL[:] = np.nan
    pt = _compute(FakeRanks(H, LL, 2))
    assert pt.best_row == -1 and np.isnan(pt.best_ll) and np.all(np.isnan(pt.best_x)) and np.all(np.isnan(pt.ll_mean))
    check_against_numpy(pt, H, LL, 0, 1)


def test_chain_ids_go_to_their_ranks():
    H, LL = _history(G=7, N=16)
    r, i = TR.owner_of([0, 3, 4, 15, 9], 16, 4)
    assert r.tolist() == [0, 0, 1, 3, 2] and i.tolist() == [0, 3, 0, 3, 1]
    for R in (1, 2, 4):
        fr = FakeRanks(H, LL, R)
        chains = [15, 0, 9, 4, 3]
        pt = _compute(fr, every=3, chains=chains)
        assert len(fr.calls) == 1 and fr.calls[0].tolist() == chains
        assert np.array_equal(pt.chain_x, H[0:7:3][:, chains]) and np.array_equal(pt.chain_ll, LL[0:7:3][:, chains])
        fr = FakeRanks(H, LL, R)
        pt = _compute(fr)
        assert fr.calls == [] and pt.chain_x.shape == (7, 0, 5) and pt.chains.shape == (0,)
    fr = FakeRanks(H, LL, 2)
    fr.n_local = 6                                 # ranks that disagree with the chain layout: chains 12 ... 15 have no owner
    with pytest.raises(RuntimeError, match=r"chains \[15\] were returned by \[0\] ranks"):
        _compute(fr, chains=[15, 0])


def test_errors_say_what_is_wrong():
    fr = FakeRanks(*_history(), R=2)
    with pytest.raises(ValueError, match=r"param_est_trace: every must be >= 1 \(got 0\)"):
        _compute(fr, every=0)
    with pytest.raises(ValueError, match=r"every must be >= 1 \(got -3\)"):
        _compute(fr, every=-3)
    with pytest.raises(TypeError, match="every must be an integer"):
        _compute(fr, every=2.5)
    with pytest.raises(ValueError, match=r"param_est_trace: chains must lie in \[0, 16\)"):
        _compute(fr, chains=[0, 16])
    with pytest.raises(ValueError, match=r"chains must lie in \[0, 16\)"):
        _compute(fr, chains=[-1])
    with pytest.raises(ValueError, match="param_est_trace: chains must be distinct"):
        _compute(fr, chains=[3, 5, 3])
    with pytest.raises(ValueError, match="chains must be None or a sequence of chain indices"):
        _compute(fr, chains=[0.5])
    with pytest.raises(ValueError, match=r"param_est_trace: n_burn must be >= 0 \(got -1\)"):
        _compute(fr, n_burn=-1)
    with pytest.raises(ValueError, match=r"param_est_trace: the window is empty \(n_burn = 353"):
        _compute(fr, n_burn=22 * 16 + 1)           # the last generation is no longer whole
    assert len(_compute(fr, n_burn=22 * 16).gen) == 1
    from bipymc_amd.samplers import DeMc
    with pytest.raises(RuntimeError, match="param_est_trace: run_mcmc first"):
        DeMc(lambda x: 0.0, n_chains=8).param_est_trace()


def test_the_bound_holds_for_shifted_sums_far_from_the_origin_and_not_for_raw_moments():
    rs = np.random.RandomState(11)
    for n in (7, 1000, 40000):
        x = 1e8 + rs.normal(size=n)
        m = math.fsum(x) / n
        var = math.fsum((np.asarray(x, dtype=np.longdouble) - np.longdouble(m)) ** 2) / n
        bm, bv = trace_bound(n, float(np.abs(x).max()), float(np.abs(x - m).max()))
        for c in (x[0], x.max(), x.min()):        # any value of the bin as the shift
            d = x - c
            s1 = s2 = 0.0
            for v in d:                            # the worst order there is: one after the other
                s1 += v
                s2 += v * v
            assert abs(c + s1 / n - m) <= bm
            assert abs((s2 - s1 * s1 / n) / n - var) <= bv
        (cnt, sm) = FakeRanks._column(x)
        n_, mean, m2 = TR.merge_moments([(np.array(cnt[0]), np.array(sm[0]), np.array(sm[1]), np.array(sm[2]))])
        assert abs(float(mean) - m) <= bm and abs(float(m2) / n - var) <= bv
        raw = float(np.sum(x * x)) / n - float(np.sum(x) / n) ** 2         # E x^2 - (E x)^2 cancels at this offset: the bound has teeth
        assert abs(raw - var) > bv
    bm, bv = trace_bound(256, 5e-320, 5e-320)
    assert bm == 2 * TINY and bv == 4 * TINY                                 # denormals: the underflow terms are all there is
