"""bipymc_amd/histograms.py without a GPU: histograms.compute driven by a NumPy stand-in for the three device calls (the same window; the
binning rule of bipymc_amd/csrc/histograms.h restated as searchsorted(edges, x, "right") - 1 with the last edge closed), on 1, 2 and 5
emulated ranks with uneven windows.  Every comparison with np.histogram / np.histogram2d / np.histogram_bin_edges is exact: counts are
integers, edges are compared bit for bit."""
import numpy as np
import pytest

from bipymc_amd import histograms as HS


def device_bins(x, e):
    """the device's rule: the largest i <= nb - 1 with e[i] <= x; -1 for NaN and values outside [e[0], e[-1]]"""
    nb = len(e) - 1
    i = np.searchsorted(e, x, side="right") - 1
    i = np.where(x == e[-1], nb - 1, i)
    with np.errstate(invalid="ignore"):
        ok = (x >= e[0]) & (x <= e[-1])
    return np.where(ok, i, -1)


class FakeRanks(object):
    """The device calls of R ranks over one super chain X (rows, dim) laid out as generations of N chains: rank r holds the chains
    [lo_r, hi_r) of every generation."""

    def __init__(self, X, N, R):
        self.X = np.asarray(X, dtype=np.float64)
        self.N = N
        cuts = np.linspace(0, N, R + 1).astype(int)
        if R > 1:
            cuts[1] = max(1, cuts[1] - 1)       # uneven
        self.cuts = cuts
        self.R = R
        self.n_burn = None
        self.seen_edges = []

    def _rows(self, r, n_burn):
        idx = np.arange(self.X.shape[0])
        chain = idx % self.N
        return self.X[(idx >= n_burn) & (chain >= self.cuts[r]) & (chain < self.cuts[r + 1])]

    def hist_range(self, n_burn):
        self.n_burn = n_burn
        out = []
        d = self.X.shape[1]
        for r in range(self.R):
            Y = self._rows(r, n_burn)
            nan = np.isnan(Y)
            lo = np.where(nan, np.inf, Y).min(axis=0) if len(Y) else np.full(d, np.inf)
            hi = np.where(nan, -np.inf, Y).max(axis=0) if len(Y) else np.full(d, -np.inf)
            out.append((len(Y), lo, hi, nan.sum(axis=0), np.isinf(Y).sum(axis=0)))
        return out

    def hist_marginals(self, dims, edges):
        self.seen_edges.append(np.array(edges))
        out = []
        for r in range(self.R):
            Y = self._rows(r, self.n_burn)
            c = np.zeros((len(dims), edges.shape[1] - 1), dtype=np.int64)
            for j, k in enumerate(dims):
                b = device_bins(Y[:, k], edges[j])
                np.add.at(c[j], b[b >= 0], 1)
            out.append(c)
        return out

    def hist_pairs(self, dims, edges2d, pa, pb):
        out = []
        nb = edges2d.shape[1] - 1
        for r in range(self.R):
            Y = self._rows(r, self.n_burn)
            c = np.zeros((len(pa), nb, nb), dtype=np.int64)
            for p, (a, b) in enumerate(zip(pa, pb)):
                ia = device_bins(Y[:, dims[a]], edges2d[a])
                ib = device_bins(Y[:, dims[b]], edges2d[b])
                ok = (ia >= 0) & (ib >= 0)
                np.add.at(c[p], (ia[ok], ib[ok]), 1)
            out.append(c)
        return out


def run(X, N, R, n_burn=0, **kw):
    f = FakeRanks(X, N, R)
    return HS.compute(f.hist_range, f.hist_marginals, f.hist_pairs, lambda x: x, n_burn, X.shape[1], **kw), f


def check_against_numpy(ph, W, bins=20, rng=None, bins2d=None):
    """W: the window (rows, dim); rng: None, (lo, hi) or one per coordinate of ph.dims"""
    bins2d = bins if bins2d is None else bins2d
    m = len(ph.dims)
    assert ph.n == len(W)
    assert ph.counts.dtype == np.int64 and ph.counts2d.dtype == np.int64 and ph.edges.dtype == np.float64
    assert ph.edges.shape == (m, bins + 1) and ph.counts.shape == (m, bins) and ph.edges2d.shape == (m, bins2d + 1)
    rr = [None] * m if rng is None else (np.tile(np.asarray(rng, dtype=float), (m, 1)) if np.ndim(rng) == 1 else np.asarray(rng, dtype=float))
    for j, k in enumerate(ph.dims):
        r = None if rr[j] is None else tuple(rr[j])
        want, e = np.histogram(W[:, k], bins, range=r)
        assert np.array_equal(ph.edges[j].view(np.uint64), np.histogram_bin_edges(W[:, k], bins, range=r).view(np.uint64))
        assert np.array_equal(ph.edges[j], e)
        assert np.array_equal(ph.counts[j], want), (k, ph.counts[j], want)
    pos = {int(k): j for j, k in enumerate(ph.dims)}
    assert ph.counts2d.shape == (len(ph.pairs), bins2d, bins2d)
    for p, (a, b) in enumerate(ph.pairs):
        ra = [tuple(ph.edges2d[pos[int(c)]][[0, -1]]) for c in (a, b)]
        want, ea, eb = np.histogram2d(W[:, a], W[:, b], bins2d, range=ra)
        assert np.array_equal(ph.edges2d[pos[int(a)]], ea) and np.array_equal(ph.edges2d[pos[int(b)]], eb)
        assert np.array_equal(ph.counts2d[p], want.astype(np.int64)), (a, b)


def sample(seed, rows, d):
    rs = np.random.RandomState(seed)
    return rs.normal(size=(rows, d)) * (1.0 + np.arange(d)) + np.arange(d) * 3.0


def test_the_stand_in_rule_is_numpys():
    """searchsorted(edges, x, "right") - 1 with the closed last edge against np.histogram and np.histogram2d: random data with values
    placed on every edge, a large offset with a tiny spread, NaN"""
    rs = np.random.RandomState(0)
    for case in range(60):
        bins = int(rs.choice([1, 2, 7, 20, 64, 1024]))
        off, sc = [(0.0, 1.0), (1e3, 1e-3), (-5.0, 100.0), (1e6, 1e-6)][case % 4]
        x = off + sc * rs.normal(size=400)
        r = (x.min(), x.max()) if case % 3 else (off - sc, off + sc)
        e = np.linspace(r[0], r[1], bins + 1)
        x = np.concatenate([x, e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), [np.nan]])
        b = device_bins(x, e)
        got = np.bincount(b[b >= 0], minlength=bins)
        assert np.array_equal(got, np.histogram(x[~np.isnan(x)], bins, range=r)[0]), case
    for case in range(20):
        bins = int(rs.choice([1, 5, 20, 64]))
        x, y = rs.normal(size=500), 1e3 + 1e-3 * rs.normal(size=500)
        ex, ey = np.linspace(x.min(), x.max(), bins + 1), np.linspace(y.min(), y.max(), bins + 1)
        x[:bins + 1], y[-bins - 1:] = ex, ey
        ia, ib = device_bins(x, ex), device_bins(y, ey)
        got = np.zeros((bins, bins), dtype=np.int64)
        np.add.at(got, (ia, ib), 1)
        assert np.array_equal(got, np.histogram2d(x, y, bins, range=[ex[[0, -1]], ey[[0, -1]]])[0].astype(np.int64))


@pytest.mark.parametrize("R", [1, 2, 5])
def test_equals_numpy_and_ranks_sum_to_the_single_rank_result(R):
    N, G, d = 50, 60, 6
    X = sample(1, N * G, d)
    one = {}
    for n_burn in (0, 7, N * 3 + 11):
        for kw in (dict(), dict(bins=7, pairs="all"), dict(bins=64, range=(-2.0, 5.0), pairs=[(0, 1), (5, 2)], bins2d=9),
                   dict(dims=[4, 1, 3], pairs=[(3, 4), (4, 3), (1, 1)], range=[(0.0, 10.0), (2.0, 3.0), (-100.0, 100.0)])):
            ph, f = run(X, N, R, n_burn, **kw)
            check_against_numpy(ph, X[n_burn:], kw.get("bins", 20), kw.get("range"), kw.get("bins2d"))
            assert all(np.array_equal(e.view(np.uint64), ph.edges.view(np.uint64)) for e in f.seen_edges)
            ref, _ = run(X, N, 1, n_burn, **kw)
            for a, b in zip(ph, ref):
                assert np.array_equal(a, b)
            if kw.get("range") is None:
                assert np.all(ph.counts.sum(axis=1) == ph.n)
            one[(n_burn, str(kw))] = ph


def test_range_rules():
    N = 20
    X = sample(2, N * 30, 4)
    X[:, 1] = 0.7                                   # a constant column: (0.2, 1.2)
    ph, _ = run(X, N, 2)
    assert ph.edges[1, 0] == 0.7 - 0.5 and ph.edges[1, -1] == 0.7 + 0.5
    check_against_numpy(ph, X)
    ph, _ = run(X, N, 2, range=(3.0, 3.0), bins=4)  # an explicit lo == hi: (2.5, 3.5)
    assert np.array_equal(ph.edges[0], np.linspace(2.5, 3.5, 5))
    check_against_numpy(ph, X, 4, (3.0, 3.0))
    with pytest.raises(ValueError, match=r"max must be larger than min in range parameter\."):
        run(X, N, 2, range=(1.0, 0.0))
    with pytest.raises(ValueError, match=r"max must be larger than min in range parameter\."):
        run(X, N, 2, range=[(0, 1), (0, 1), (2, 1), (0, 1)])
    for bad in ((0.0, np.inf), (-np.inf, 0.0), (np.nan, 1.0), (0.0, np.nan)):
        with pytest.raises(ValueError, match=r"supplied range of \[.*\] is not finite"):
            run(X, N, 2, range=bad)
    with pytest.raises(ValueError, match="range must be"):
        run(X, N, 2, range=[(0, 1), (0, 1)])
    # non-finite data: an error under range=None (NumPy's wording), counted nowhere under a given range
    for val, text in ((np.nan, r"autodetected range of \[nan, nan\] is not finite"), (np.inf, r"autodetected range of \[.*, inf\] is not finite"),
                      (-np.inf, r"autodetected range of \[-inf, .*\] is not finite")):
        Y = X.copy()
        Y[N * 7 + 3, 2] = val
        with pytest.raises(ValueError, match=text):
            run(Y, N, 2)
        with pytest.raises(ValueError) as ei:
            np.histogram(Y[:, 2], 20)
        with pytest.raises(ValueError) as ej:
            run(Y, N, 1, dims=[2])
        assert str(ei.value) == str(ej.value)
        ph, _ = run(Y, N, 2, dims=[0, 1, 3])        # the other columns are fine
        check_against_numpy(ph, Y)
        ph, _ = run(Y, N, 2, range=(-3.0, 9.0), pairs=[(2, 0)])
        check_against_numpy(ph, np.where(np.isnan(Y), 1e300, Y), 20, (-3.0, 9.0))      # (np.histogram2d refuses NaN; outside = nowhere)
        assert ph.counts[2].sum() <= ph.n - 1
        Y[:N * 7 + 4, 2] = val                      # ... and gone once the window starts behind it
        ph, _ = run(Y, N, 2, n_burn=N * 7 + 4)
        check_against_numpy(ph, Y[N * 7 + 4:])


def test_edges_are_numpys_bit_for_bit():
    rs = np.random.RandomState(3)
    for off, sc in ((0.0, 1.0), (1e3, 1e-3), (-1e8, 1.0), (0.1, 1e-12), (0.0, 5e-324 * 1000)):
        X = off + sc * rs.uniform(size=(40 * 10, 3))
        for bins in (1, 3, 20, 1024):
            try:
                np.histogram_bin_edges(X[:, 0], bins)
            except ValueError as e:                 # (1024 bins over a thousand denormal steps)
                with pytest.raises(ValueError, match="Too many bins for data range") as ei:
                    run(X, 40, 2, bins=bins)
                assert str(ei.value) == str(e)
                continue
            ph, _ = run(X, 40, 2, bins=bins)
            for k in range(3):
                assert np.array_equal(ph.edges[k].view(np.uint64), np.histogram_bin_edges(X[:, k], bins).view(np.uint64))
            check_against_numpy(ph, X, bins)


def test_dims_and_pairs():
    X = sample(4, 30 * 20, 5)
    ph, _ = run(X, 30, 2, dims=[3, 0, 4], pairs="all")
    assert np.array_equal(ph.dims, [3, 0, 4])
    assert np.array_equal(ph.pairs, [(3, 0), (3, 4), (0, 4)])       # every a < b by position in dims, lexicographic
    check_against_numpy(ph, X)
    ph, _ = run(X, 30, 1, pairs="all")
    assert np.array_equal(ph.pairs, [(a, b) for a in range(5) for b in range(a + 1, 5)])
    ph, _ = run(X, 30, 1)
    assert ph.pairs.shape == (0, 2) and ph.counts2d.shape == (0, 20, 20) and ph.edges2d.shape == (5, 21)
    ph, _ = run(X, 30, 1, pairs=[(1, 0)])
    assert np.array_equal(ph.counts2d[0], run(X, 30, 1, pairs=[(0, 1)])[0].counts2d[0].T)
    for bad in ([0, 0], [5], [-1], [], [[0, 1]], [0.5], "all"):
        with pytest.raises(ValueError, match="dims"):
            run(X, 30, 1, dims=bad)
    for bad in ([(0, 5)], [(0, 1, 2)], [0, 1], "every", [(0.5, 1)]):
        with pytest.raises(ValueError, match="pair"):
            run(X, 30, 1, pairs=bad)
    with pytest.raises(ValueError, match="must be in dims"):
        run(X, 30, 1, dims=[0, 1], pairs=[(0, 2)])


def test_density():
    X = sample(5, 30 * 20, 3)
    X[:, 1] = 2.0
    ph, _ = run(X, 30, 2, bins=11)
    dens = ph.density()
    for k in range(3):
        assert np.array_equal(dens[k], np.histogram(X[:, k], 11, density=True)[0])
    ph, _ = run(X, 30, 2, bins=5, range=(1e3, 2e3))            # nothing inside: NaN, as NumPy
    with np.errstate(invalid="ignore"):
        want = np.histogram(X[:, 0], 5, range=(1e3, 2e3), density=True)[0]
    assert np.isnan(want).all() and np.isnan(ph.density()).all()


def test_bin_limits_and_errors():
    X = sample(6, 10 * 4, 3)
    check_against_numpy(run(X, 10, 1, bins=1024)[0], X, 1024)
    check_against_numpy(run(X, 10, 1, bins=1024, pairs="all", bins2d=64)[0], X, 1024, None, 64)
    for bins in (0, -1, 1025):
        with pytest.raises(ValueError, match=r"bins = -?\d+ is outside the supported 1 \.\.\. 1024"):
            run(X, 10, 1, bins=bins)
    for b2 in (0, 65):
        with pytest.raises(ValueError, match=r"bins2d = \d+ is outside the supported 1 \.\.\. 64"):
            run(X, 10, 1, pairs="all", bins2d=b2)
    with pytest.raises(ValueError, match=r"bins2d = 100 is outside the supported 1 \.\.\. 64"):
        run(X, 10, 1, bins=100, pairs="all")        # bins2d defaults to bins
    assert run(X, 10, 1, bins=100)[0].counts.shape == (3, 100)
    with pytest.raises(TypeError):
        run(X, 10, 1, bins=2.5)
    with pytest.raises(ValueError, match="window is empty"):
        run(X, 10, 2, 40)
    with pytest.raises(ValueError, match="window is empty"):
        run(X, 10, 1, 10 ** 9)
    with pytest.raises(ValueError, match="n_burn must be >= 0"):
        run(X, 10, 1, -1)
    check_against_numpy(run(X, 10, 2, 39)[0], X[39:])          # a window of one row


def test_exported_from_the_package():
    import bipymc_amd
    assert bipymc_amd.PosteriorHistograms is HS.PosteriorHistograms
    assert bipymc_amd.PosteriorHistograms._fields == ("dims", "edges", "counts", "pairs", "edges2d", "counts2d", "n")
