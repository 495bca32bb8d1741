"""Host side of the posterior quantiles (bipymc_amd/quantiles.py): the order-preserving key map, NumPy's target ranks and interpolation
restated, and the collective radix-select driver against np.quantile with a NumPy stand-in for the two engine calls, over 1-3 emulated
ranks.  Every comparison is np.array_equal(..., equal_nan=True) against np.quantile."""
import numpy as np
import pytest

from bipymc_amd import quantiles as Q

QS = [0.0, 1.0, 0.5, 1.0 / 3.0, 0.05, 0.95]


def _doubles(rs, n):
    x = rs.normal(size=n) * 10.0 ** rs.randint(-300, 300, size=n)
    bits = rs.randint(0, 2 ** 63, size=n, dtype=np.int64).astype(np.uint64) | (rs.randint(0, 2, size=n).astype(np.uint64) << np.uint64(63))
    raw = bits.view(np.float64)
    raw = raw[~np.isnan(raw)]
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1.7976931348623157e308, -1.7976931348623157e308,
                        1.0, -1.0])
    return np.concatenate([x, raw, special])


def test_key_map_preserves_order_and_inverts():
    rs = np.random.RandomState(0)
    x = _doubles(rs, 5000)
    k = Q.to_key(x)
    o = np.lexsort((~np.signbit(x), x))                  # numeric order, -0.0 before 0.0
    ks = k[o]
    assert np.all(ks[1:] >= ks[:-1])                      # numeric order -> key order
    xs = x[o]
    strict = xs[1:] > xs[:-1]
    assert np.all(ks[1:][strict] > ks[:-1][strict])
    assert np.array_equal(Q.from_key(k).view(np.uint64), x.view(np.uint64))     # bit-exact inverse, -0.0 included
    assert Q.to_key(np.array([-0.0]))[0] < Q.to_key(np.array([0.0]))[0]
    nans = np.array([np.nan, -np.nan, np.uint64(0x7FF0000000000001).view(np.float64), np.uint64(0xFFF8000000000123).view(np.float64)])
    kn = Q.to_key(nans)
    assert np.all(kn == Q.NAN_KEY) and np.all(kn > Q.to_key(np.array([np.inf]))[0])
    assert np.isnan(Q.from_key(kn)).all()


def _via_targets(X, q):
    """np.quantile through Q.targets / Q.finish with the order statistics taken from a sorted copy"""
    X = np.asarray(X, dtype=np.float64)
    q = Q.check_q(q)
    S = np.sort(X, axis=0)
    return Q.finish(X.shape[0], q, lambda rr: S[np.asarray(rr)], np.isnan(X).any(axis=0))


@pytest.mark.parametrize("n", [1, 2, 3, 7, 1000, 12345])
def test_targets_and_interpolation_match_numpy(n):
    rs = np.random.RandomState(n)
    X = rs.normal(size=(n, 4))
    X[:, 1] = np.round(X[:, 1] * 2.0)                      # ties
    if n >= 3:
        X[rs.randint(0, n, size=max(1, n // 5)), 2] = np.inf
        X[rs.randint(0, n, size=max(1, n // 7)), 2] = -np.inf
    X[rs.randint(0, n), 3] = np.nan
    qs = np.concatenate([QS, rs.uniform(size=200)])
    got = _via_targets(X, qs)
    assert np.array_equal(got, np.quantile(X, qs, axis=0), equal_nan=True)
    for q in QS:
        assert np.array_equal(_via_targets(X, q), np.quantile(X, q, axis=0), equal_nan=True)
        assert np.array_equal(_via_targets(X, [q]), np.quantile(X, [q], axis=0), equal_nan=True)
    for q in (0, 1, [0, 1], np.float32(0.3), np.array([0.25, 0.75], dtype=np.float32)):
        assert np.array_equal(_via_targets(X, q), np.quantile(X, q, axis=0), equal_nan=True), q


def test_numpy_quirks():
    X = np.array([[np.inf], [np.inf], [1.0]])
    assert np.array_equal(_via_targets(X, [0.5, 1.0]), np.quantile(X, [0.5, 1.0], axis=0), equal_nan=True)
    assert np.isnan(_via_targets(X, [0.5, 1.0])).all()
    Z = np.array([[-0.0], [0.0], [-0.0], [0.0]])
    assert np.array_equal(_via_targets(Z, QS), np.quantile(Z, QS, axis=0))


def test_bad_q_raises_numpys_message():
    for q in (-0.1, 1.5, [0.5, 2.0], np.nan):
        with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
            Q.check_q(q)
        with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
            np.quantile(np.zeros(3), q)


class StandIn(object):
    """the two engine calls in NumPy over one rank's chains [lo, hi) of a (G, N, d) history"""

    def __init__(self, H, lo, hi):
        self.H, self.lo, self.hi = H, lo, hi
        self.win = None
        self.calls = 0

    def begin(self, n_burn):
        G, N, d = self.H.shape
        g0, first = n_burn // N, n_burn % N
        rows = []
        for g in range(min(g0, G), G):
            c0 = self.lo if g > g0 else max(self.lo, min(first, self.hi))
            rows.append(self.H[g, c0:self.hi])
        self.win = Q.to_key(np.concatenate(rows, axis=0) if rows else np.zeros((0, d)))
        return self.win.shape[0]

    def histogram(self, pk, pv, bits):
        self.calls += 1
        hist = np.zeros((len(pk), 256), dtype=np.uint64)
        nn = np.zeros(len(pk), dtype=np.int64)
        for j, (k, p) in enumerate(zip(pk, pv)):
            col = self.win[:, int(k)]
            m = np.ones(len(col), dtype=bool) if bits == 0 else (col >> np.uint64(64 - bits)) == p
            dig = ((col[m] >> np.uint64(56 - bits)) & np.uint64(255)).astype(np.int64)
            hist[j] = np.bincount(dig, minlength=256).astype(np.uint64)
            nn[j] = int(np.sum(col[m] == Q.NAN_KEY))
        return hist, nn


def _world(H, n_burn, q, R):
    G, N, d = H.shape
    cuts = np.linspace(0, N, R + 1).astype(int)
    ranks = [StandIn(H, cuts[r], cuts[r + 1]) for r in range(R)]
    got = Q.compute(lambda nb: [e.begin(nb) for e in ranks], lambda a, b, c: [e.histogram(a, b, c) for e in ranks], lambda x: x, n_burn, q,
                    dim=d)
    assert all(e.calls == Q.PASSES for e in ranks)
    return got


def _history(G, N, d, seed):
    rs = np.random.RandomState(seed)
    H = rs.normal(size=(G, N, d))
    if d > 1:
        H[:, :, 1] = np.round(H[:, :, 1])                   # heavy ties
    if d > 2:
        H[:, :, 2] = 0.75                                   # a constant column
    if d > 3:
        H[: G // 2, rs.randint(0, N), 3] = H[0, 0, 3]       # a stuck chain
    if d > 4:
        H[1, 3 % N, 4] = np.nan
    if d > 5:
        H[0, :, 5] = np.inf
        H[1, :2, 5] = -np.inf
        H[2, :, 5] = -0.0
        H[3, :, 5] = 0.0
    return H


@pytest.mark.parametrize("R", [1, 2, 3])
def test_driver_matches_numpy_across_emulated_ranks(R):
    H = _history(9, 12, 7, seed=R)
    G, N, d = H.shape
    qs = np.concatenate([QS, np.random.RandomState(3).uniform(size=20)])
    for n_burn in (0, 5, N, N * 3 + 7, G * N - 1):
        want = np.quantile(H.reshape(-1, d)[n_burn:], qs, axis=0)
        assert np.array_equal(_world(H, n_burn, qs, R), want, equal_nan=True), n_burn
    for q in (0.5, 0, 1, [0.0, 1.0]):
        assert np.array_equal(_world(H, N + 2, q, R), np.quantile(H.reshape(-1, d)[N + 2:], q, axis=0), equal_nan=True)


def test_driver_edge_shapes():
    H = _history(3, 4, 1, seed=9)                        # d = 1
    assert np.array_equal(_world(H, 0, QS, 2), np.quantile(H.reshape(-1, 1), QS, axis=0))
    H = _history(4, 3, 6, seed=10)
    n_burn = 4 * 3 - 1                                    # n = 1
    assert np.array_equal(_world(H, n_burn, QS, 1), np.quantile(H.reshape(-1, 6)[n_burn:], QS, axis=0), equal_nan=True)
    X = np.full((50, 8, 2), 3.0)
    X[:, :, 1] = np.repeat(np.arange(5.0), 80).reshape(50, 8)
    assert np.array_equal(_world(X, 17, QS, 3), np.quantile(X.reshape(-1, 2)[17:], QS, axis=0))


def test_driver_errors():
    H = _history(3, 4, 2, seed=1)
    with pytest.raises(ValueError, match="window is empty"):
        _world(H, 12, QS, 2)
    with pytest.raises(ValueError, match="window is empty"):
        _world(H, 40, QS, 1)
    with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
        _world(H, 0, [0.5, 1.01], 1)
    with pytest.raises(ValueError, match="n_burn must be >= 0"):
        _world(H, -1, QS, 1)
