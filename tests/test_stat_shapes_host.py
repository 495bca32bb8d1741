"""tests/_stat_shape_cases.py without a GPU: every case is on the branch it claims (the launch arithmetic restated from sampler.hip against
the tables), and the REFERENCE alone is sound on these inputs -- integer sums that float64 holds exactly, np.quantile through the NumPy
stand-in of the two quantile calls.  A failure of tests/test_gpu_stat_shapes.py then points at a kernel."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _stat_shape_cases as S  # noqa: E402
from bipymc_amd import quantiles as Q  # noqa: E402
from test_quantiles_host import StandIn  # noqa: E402


def test_every_case_takes_the_path_it_claims():
    S.assert_cov_paths()
    S.assert_moments_paths()
    S.assert_quantile_paths()
    S.assert_histogram_paths()
    S.assert_trace_paths()


def test_constants_are_the_ones_the_issue_counted_with():
    """the shapes were chosen for these values; another value moves the cases, and the tables above say where to"""
    assert (S.COV_MAX_T, S.COV_BLK, S.COV_UNR) == (7, 4, 4)
    assert (S.QS_THREADS, S.QS_SLOTS, S.QS_UNR) == (256, 32, 4)
    assert (S.HS_THREADS, S.HS_UNR, S.HS_TILE_PAIRS, S.HS_LDS_PAIRS) == (256, 4, 64, 32 * 1024)
    assert (S.TR_THREADS, S.TR_UNR, S.MOM_THREADS) == (256, 4, 256)


def _integer_shapes():
    """(G, N, d) of every covariance, moment and trace case"""
    out = [(S.COV_G, S.COV_N, d) for d in list(S.COV_SINGLE) + list(S.COV_BLOCKED)]
    out += [(G, N, d) for d, N, G, _ in S.COV_LONG]
    out += [(S.MOM_G, S.MOM_N, d) for d in S.MOM_DIMS]
    out += [(S.TR_G, S.TR_N, d) for d in S.TR_DIMS]
    out += [(c["G"], c["N"], c["d"]) for c in (S.TR_PARTS, S.TR_EMPTY)]
    return out


def test_integer_sums_are_exact_whatever_the_order():
    """|x|, |c| <= 8 integers: |x - c| <= 16, so every partial sum any order of additions can form is an integer of magnitude at most
    rows * 16^2, below 2^53"""
    for G, N, d in _integer_shapes():
        assert G * N * 16 ** 2 < 2 ** 53
    for G, N, d in sorted(set(_integer_shapes()), key=lambda s: s[0] * s[1] * s[2])[:12]:
        H, X, c = S.integer_history(G, N, d, seed=d)
        assert H.shape == (G, N, d) and np.array_equal(X, H[-1])
        for a in (H, c):
            assert a.dtype == np.float64 and np.array_equal(a, np.round(a)) and np.abs(a).max() <= 8
        assert len(np.unique(H)) == 17 or H.size < 200          # every value of [-8, 8] occurs: no constant pattern
    G, N, d = S.COV_G, S.COV_N, min(S.COV_SINGLE)
    for d in (min(S.COV_SINGLE), 17):
        H, _, c = S.integer_history(G, N, d, seed=d)
        R = H.reshape(-1, d) - c
        exact = R.astype(np.int64).astype(object)
        assert np.array_equal((R.T @ R).astype(object), exact.T.dot(exact))       # float64 against Python integers
        assert np.array_equal(R.sum(axis=0).astype(object), exact.sum(axis=0))


class Spy(StandIn):
    """records the requests of every pass"""

    def __init__(self, *a):
        StandIn.__init__(self, *a)
        self.seen = []

    def histogram(self, pk, pv, bits):
        hist, nn = StandIn.histogram(self, pk, pv, bits)
        self.seen.append((np.array(pk), bits, hist))
        return hist, nn


@pytest.fixture(scope="module")
def qhist():
    return S.quantile_history(S.QH_G, S.QH_N, S.QH_SEED)


def test_quantile_history_is_what_its_columns_say(qhist):
    R = qhist.reshape(-1, 6)
    K = Q.to_key(R)
    for k in (0, 4):                                          # six leading bytes shared, the last two differ
        assert len(np.unique(K[:, k] >> np.uint64(16))) == 1 and len(np.unique(K[:, k] >> np.uint64(8))) > 100
    assert R[:, 0].min() >= 1.0 and R[:, 4].max() <= -3.0 and np.all(np.signbit(R[:, 4]))
    z = R[:, 1] == 0.0
    assert np.signbit(R[z, 1]).any() and not np.signbit(R[z, 1]).all()
    assert np.abs(R[:, 1]).max() <= 300 * 5e-324 and (R[:, 1] > 0).any() and (R[:, 1] < 0).any()
    assert (R[:, 2] < 2.0).any() and (R[:, 2] > 2.0).any()
    assert set(np.unique(R[:, 3])) <= set(S.SPECIALS) and np.isinf(R[:, 3]).any()
    assert np.signbit(R[-2, 1]) and not np.signbit(R[-1, 1]) and R[-2, 1] == 0.0 == R[-1, 1]      # both zeros in the two-row window


@pytest.mark.parametrize("n_burn", S.QH_BURNS)
def test_quantile_reference_is_sound_and_crosses_tiles(qhist, n_burn):
    G, N, d = qhist.shape
    e = Spy(qhist, 0, N)
    W = qhist.reshape(-1, d)[n_burn:]
    with np.errstate(invalid="ignore"):
        want = np.quantile(W, S.Q41, axis=0)
        got = Q.compute(lambda nb: [e.begin(nb)], lambda a, b, c: [e.histogram(a, b, c)], lambda x: x, n_burn, S.Q41, dim=d)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(Q.compute(lambda nb: [e.begin(nb)], lambda a, b, c: [e.histogram(a, b, c)], lambda x: x, n_burn, 0.5, dim=d),
                          np.quantile(W, 0.5, axis=0), equal_nan=True)
    if len(W) < 100:
        return
    # more than QS_SLOTS slots on one coordinate in some pass: that coordinate's slots span tiles, one of which starts inside it
    most = max((int(np.bincount(pk).max()), i) for i, (pk, bits, _) in enumerate(e.seen[:Q.PASSES]))
    assert most[0] > S.QS_SLOTS, most
    pk = e.seen[most[1]][0]
    assert S.starts_inside_a_coordinate(pk, S.quantile_tiles(pk))
    # the last pass decides: a slot with more than one occupied bin at bits = 56
    pk, bits, hist = e.seen[Q.PASSES - 1]
    assert bits == 56 and ((hist > 0).sum(axis=1) > 1).any()
    assert ((hist[pk == 0] > 0).sum(axis=1) > 1).any()


@pytest.mark.parametrize("d", S.Q_SPAN_DIMS)
def test_span_cut_cases_reference(d):
    H = S.shifted_normal_history(6, 8, d, S.QH_SEED)
    e = Spy(H, 0, 8)
    got = Q.compute(lambda nb: [e.begin(nb)], lambda a, b, c: [e.histogram(a, b, c)], lambda x: x, 5, 0.25, dim=d)
    assert np.array_equal(got, np.quantile(H.reshape(-1, d)[5:], 0.25, axis=0))
    pk0 = e.seen[0][0]
    assert np.array_equal(pk0, np.arange(d))                  # pass 0: one slot per coordinate
    assert [t[3] for t in S.quantile_tiles(pk0)] == S.Q_SPAN_TILES[d]


def test_direct_slot_requests_count_something():
    """the hand-built requests are not vacuous: all but the prefix no key carries find keys, and that one finds none"""
    for name, H, n_burn, pk, pv, bits, _ in S.direct_slot_cases():
        e = StandIn(H, 0, H.shape[1])
        e.begin(n_burn)
        hist, nn = e.histogram(pk, pv, bits)
        if name == "a prefix no key carries":
            assert not hist.any()
        else:
            assert hist.any(), name
        if "slots on one coordinate" in name or name == "the last byte of column 0":
            assert (hist.sum(axis=1) > 0).all(), name


def test_pair_tiling_restated():
    """64 pairs over 128 slots in one tile; with every pair of 24 coordinates the same slot sits in many tiles"""
    pa, pb = zip(*S.HP_WIDE["pairs"])
    tp_max, tiles = S.pair_tiles(pa, pb, S.HP_WIDE["bins2d"])
    assert [(p0, n, len(sl)) for p0, n, sl in tiles] == [(0, 64, 128)]
    pa, pb = zip(*S.all_pairs(S.HP_ALL["d"]))
    for bins2d in S.HP_ALL_BINS:
        _, tiles = S.pair_tiles(pa, pb, bins2d)
        assert sum(n for _, n, _ in tiles) == 276 and all(2 <= len(sl) <= 2 * n for _, n, sl in tiles)
        assert sum(1 for _, _, sl in tiles if 23 in sl) > 1
    for pairs in S.HP_ODD_PAIRS.values():
        pa, pb = zip(*pairs)
        _, tiles = S.pair_tiles(pa, pb, 20)
        assert len(tiles) == 1 and len(tiles[0][2]) < 2 * len(pairs)       # a slot shared inside the tile
