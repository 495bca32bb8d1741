"""The covariance, raw-moment, quantile, histogram and trace kernels of the resident history at every shape where the kernel or its launch
code changes path (tests/_stat_shape_cases.py: the tables, the inputs, and why each case is on its branch;
tests/test_stat_shapes_host.py checks the tables and the references without a GPU).  Histories are installed with set_history; every
comparison is np.array_equal against integer sums that float64 holds exactly, or against NumPy's own values.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _stat_shape_cases as S  # noqa: E402
from _history_cases import _engine  # noqa: E402
from bipymc_amd import histograms as HS  # noqa: E402
from bipymc_amd import quantiles as Q  # noqa: E402
from test_histograms_host import check_against_numpy  # noqa: E402
from test_quantiles_host import StandIn  # noqa: E402

pytestmark = pytest.mark.gpu


def _installed(H, X=None):
    G, N, d = H.shape
    e = _engine(N, d)
    e.set_history(H, H[-1] if X is None else X)
    return e


# ---- covariance and raw moments ----------------------------------------------------------------------------------------------------------
def _check_cov(e, R, n_burn, c):
    cnt, s1, s2 = e.reduce_cov(n_burn, c)
    D = R[n_burn:] - c
    assert cnt == len(D)
    assert np.array_equal(s1, D.sum(axis=0)), (n_burn, np.nonzero(s1 != D.sum(axis=0))[0][:8])
    want = D.T @ D
    bad = np.argwhere(s2 != want)
    assert len(bad) == 0, (n_burn, len(bad), bad[:8].tolist())
    assert np.array_equal(s2, s2.T)


@pytest.mark.parametrize("d", sorted(S.COV_SINGLE) + sorted(S.COV_BLOCKED))
def test_covariance_equals_the_integer_sums_at_every_tile_count(d):
    """cov_partial_kernel<T, true> for every T = 1 ... 7 with a full last tile and with a last tile of one column; the blocked form with one
    block pair, with a third block of a single column, and with six block pairs (cov_block_pair past its first row); windows of 40, 37, 23, 5
    and 2 rows that start off a multiple of 4; the zero centre and an integer one"""
    H, X, c = S.integer_history(S.COV_G, S.COV_N, d, seed=100 + d)
    e = _installed(H, X)
    R = H.reshape(-1, d)
    try:
        for n_burn in S.COV_BURNS:
            _check_cov(e, R, n_burn, np.zeros(d))
            _check_cov(e, R, n_burn, c)
    finally:
        e.close()


@pytest.mark.parametrize("d,N,G,n_burn", sorted(S.COV_LONG))
def test_covariance_over_a_second_ragged_trip_round_the_loop(d, N, G, n_burn):
    """ceil(rows / 4) > COV_UNR * nbx: the workgroups load the next step while they multiply, go round again, and end on a step of which
    only some groups, and of the last group only some rows, exist"""
    H, X, c = S.integer_history(G, N, d, seed=d)
    e = _installed(H, X)
    R = H.reshape(-1, d)
    try:
        _check_cov(e, R, n_burn, np.zeros(d))
        _check_cov(e, R, n_burn, c)
    finally:
        e.close()


@pytest.mark.parametrize("d", sorted(S.MOM_DIMS))
def test_raw_moments_equal_the_integer_sums(d):
    """moments_partial_kernel where ld / 2 pairs fill the block exactly (511, 512), leave one pair for a second pass over the columns (513) or
    leave most of the block to further rows (1, 2, 3); a window of two blocks, one of 64 + 1 rows and one shorter than 64 rows.  The shift is
    chain 0's state, an integer here"""
    H, X, _ = S.integer_history(S.MOM_G, S.MOM_N, d, seed=200 + d)
    e = _installed(H, X)
    R = H.reshape(-1, d)
    try:
        for n_burn, rows in S.MOM_BURNS.items():
            cnt, s1, s2, sh = e.reduce_moments(n_burn)
            assert cnt == rows
            assert np.array_equal(sh, X[0])
            D = R[n_burn:] - sh
            assert np.array_equal(s1, D.sum(axis=0)), (n_burn, np.nonzero(s1 != D.sum(axis=0))[0][:8])
            assert np.array_equal(s2, (D * D).sum(axis=0)), (n_burn, np.nonzero(s2 != (D * D).sum(axis=0))[0][:8])
    finally:
        e.close()


# ---- quantiles ------------------------------------------------------------------------------------------------------------------------------
def _quantiles(e, n_burn, q):
    return Q.compute(e.quantile_begin, e.quantile_histogram, Q.single_process_allgather, n_burn, q, dim=e.dim)


@pytest.fixture(scope="module")
def qhist():
    return S.quantile_history(S.QH_G, S.QH_N, S.QH_SEED)


def test_41_quantiles_follow_more_slots_than_a_tile_holds(qhist):
    """41 quantiles: the normal column has more than QS_SLOTS slots from the third pass on, so its slots span tiles and a tile starts inside
    it; column 0 and column 4 are decided by the last two bytes only (bits = 48, 56); denormals either side of zero with both zeros, keys
    either side of an exponent change, and the infinities, where NumPy's interpolation gives NaN.  Windows down to 2 rows and 1 row"""
    G, N, d = qhist.shape
    e = _installed(qhist)
    R = qhist.reshape(-1, d)
    try:
        for n_burn in S.QH_BURNS:
            for q in (S.Q41, 0.5):
                with np.errstate(invalid="ignore"):
                    want = np.quantile(R[n_burn:], q, axis=0)
                    got = _quantiles(e, n_burn, q)
                assert np.array_equal(got, want, equal_nan=True), (n_burn, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8].tolist())
    finally:
        e.close()


@pytest.mark.parametrize("d", S.Q_SPAN_DIMS)
def test_one_quantile_where_the_coordinate_span_cuts_the_tiles(d):
    """one slot per coordinate in pass 0: tiles of 32 coordinates, a last tile of one"""
    H = S.shifted_normal_history(6, 8, d, S.QH_SEED)
    e = _installed(H)
    try:
        for n_burn, q in ((5, 0.25), (0, 0.5)):
            assert np.array_equal(_quantiles(e, n_burn, q), np.quantile(H.reshape(-1, d)[n_burn:], q, axis=0))
    finally:
        e.close()


def test_hand_built_slot_lists_through_the_c_abi():
    """bpm_quantile_histogram against the NumPy stand-in of the same window, hist and n_nan value for value: one slot; 33 and 65 slots on
    one coordinate; slots whose coordinates are 31 and 32 apart; a tile that starts inside a coordinate and goes on to another; a prefix no
    key carries; the last byte (bits = 56)"""
    engines = {}
    try:
        for name, H, n_burn, pk, pv, bits, _ in S.direct_slot_cases():
            if id(H) not in engines:
                engines[id(H)] = _installed(H)
            e = engines[id(H)]
            ref = StandIn(H, 0, H.shape[1])
            assert e.quantile_begin(n_burn) == ref.begin(n_burn)
            hist, nn = e.quantile_histogram(pk, pv, bits)
            want, want_nn = ref.histogram(pk, pv, bits)
            assert np.array_equal(hist, want), (name, np.argwhere(hist != want)[:8].tolist())
            assert np.array_equal(nn, want_nn), name
    finally:
        for e in engines.values():
            e.close()


def test_rows_where_a_second_workgroup_along_the_rows_appears():
    """d = 2: kw = 2, cpw = 128, QS_UNR * cpw = 512 rows per sweep; 2048 rows are one workgroup's, 2049 rows two workgroups'"""
    H = S.shifted_normal_history(S.Q_ROWS_G, S.Q_ROWS_N, 2, 3)
    e = _installed(H)
    R = H.reshape(-1, 2)
    try:
        for n_burn, (rows, _) in S.Q_ROWS_BURNS.items():
            ref = StandIn(H, 0, S.Q_ROWS_N)
            assert e.quantile_begin(n_burn) == ref.begin(n_burn) == rows
            pk, pv = np.array([0, 1], dtype=np.int32), np.zeros(2, dtype=np.uint64)
            hist, nn = e.quantile_histogram(pk, pv, 0)
            want, want_nn = ref.histogram(pk, pv, 0)
            assert np.array_equal(hist, want) and np.array_equal(nn, want_nn) and int(hist[0].sum()) == rows
            assert np.array_equal(_quantiles(e, n_burn, [0.0, 0.5, 1.0]), np.quantile(R[n_burn:], [0.0, 0.5, 1.0], axis=0))
    finally:
        e.close()


# ---- histograms -----------------------------------------------------------------------------------------------------------------------------
def _hist(e, n_burn=0, **kw):
    return HS.compute(e.hist_range, e.hist_marginals, e.hist_pairs, HS.single_process_allgather, n_burn, e.dim, **kw)


def _normal_history(G, N, d, seed):
    rs = np.random.RandomState(seed)
    return rs.normal(size=(G, N, d)) * (1.0 + np.arange(d) % 7) + np.arange(d) % 5


def test_a_full_pair_tile_of_64_pairs_over_128_slots():
    """one tile of HS_TILE_PAIRS pairs over 128 distinct slots: cpw1 = 2, chunks of rc = 8 rows; windows of 1, rc - 1, rc and rc + 1 rows"""
    c = S.HP_WIDE
    H = _normal_history(c["G"], c["N"], c["d"], 31)
    e = _installed(H)
    R = H.reshape(-1, c["d"])
    try:
        for rows in S.HP_WIDE_ROWS:
            n_burn = len(R) - rows
            ph = _hist(e, n_burn, pairs=c["pairs"], bins2d=c["bins2d"])
            check_against_numpy(ph, R[n_burn:], 20, None, c["bins2d"])
    finally:
        e.close()


def test_every_pair_of_24_coordinates_in_ragged_tiles():
    """276 pairs in tiles of 56 + a last one of 52 (bins2d = 5, 11: the pair limit binds; 12: the LDS does), of 3 and of 2 pairs (46, 64):
    the same slot sits in many tiles.  Also a coordinate paired with itself and a pair given twice"""
    c = S.HP_ALL
    H = _normal_history(c["G"], c["N"], c["d"], 32)
    e = _installed(H)
    R = H.reshape(-1, c["d"])
    try:
        for bins2d in S.HP_ALL_BINS:
            ph = _hist(e, 3, pairs="all", bins2d=bins2d)
            assert len(ph.pairs) == 276
            check_against_numpy(ph, R[3:], 20, None, bins2d)
        for pairs in S.HP_ODD_PAIRS.values():
            ph = _hist(e, 0, pairs=pairs)
            assert np.array_equal(ph.pairs, pairs)
            check_against_numpy(ph, R)
    finally:
        e.close()


def test_marginal_tiles_with_a_short_last_tile():
    """200 coordinates at 20 bins: tiles of 165 and 35 slots; 7 coordinates at 1024 bins: tiles of 3, 3 and 1 slots"""
    H = _normal_history(6, 8, 200, 33)
    e = _installed(H)
    R = H.reshape(-1, 200)
    try:
        for n_burn in (0, 5):
            check_against_numpy(_hist(e, n_burn, bins=20), R[n_burn:], 20)
            ph = _hist(e, n_burn, bins=1024, dims=list(range(7)))
            check_against_numpy(ph, R[n_burn:], 1024)
    finally:
        e.close()


@pytest.mark.parametrize("d", sorted(S.HR_DIMS))
def test_range_over_one_full_column_tile_and_a_second_tile_of_two(d):
    """ld = 256: one column tile, one row per sweep of the block (cpw = 1); ld = 258: a second tile with two busy lanes.  A NaN, a +inf and a
    -inf sit in the last two columns"""
    H = _normal_history(7, 5, d, 34)
    H[2, 1, d - 1] = np.nan
    H[3, 4, d - 1] = np.inf
    H[5, 0, d - 2] = -np.inf
    H[6, 4, d - 2] = np.nan
    e = _installed(H)
    R = H.reshape(-1, d)
    try:
        for n_burn in (0, 3, 14):
            W = R[n_burn:]
            cnt, lo, hi, n_nan, n_inf = e.hist_range(n_burn)
            nan = np.isnan(W)
            assert cnt == len(W)
            assert np.array_equal(lo, np.where(nan, np.inf, W).min(axis=0)) and np.array_equal(hi, np.where(nan, -np.inf, W).max(axis=0))
            assert np.array_equal(n_nan, nan.sum(axis=0)) and np.array_equal(n_inf, np.isinf(W).sum(axis=0))
    finally:
        e.close()


# ---- traces ---------------------------------------------------------------------------------------------------------------------------------
def _check_traces(e, H, g_lo, g_hi, every):
    """the coordinate records only (the ln-likes are no integers): counts, the shift = the bin's first row, S1, S2, min, max"""
    G, N, d = H.shape
    counts, sums = e.trace_bins(g_lo, g_hi, every)[:2]
    ev = min(every, g_hi - g_lo)
    T = -(-(g_hi - g_lo) // ev)
    assert counts.shape == (2, T, d) and sums.shape == (5, T, d)
    for t in range(T):
        ga = g_lo + t * ev
        B = H[ga:min(ga + ev, g_hi)].reshape(-1, d)
        D = B - B[0]
        where = (d, g_lo, every, t)
        assert np.all(counts[0, t] == len(B)) and not counts[1, t].any(), where
        assert np.array_equal(sums[0, t], B[0]), where
        assert np.array_equal(sums[1, t], D.sum(axis=0)), where
        assert np.array_equal(sums[2, t], (D * D).sum(axis=0)), where
        assert np.array_equal(sums[3, t], B.min(axis=0)) and np.array_equal(sums[4, t], B.max(axis=0)), where


@pytest.mark.parametrize("d", sorted(S.TR_DIMS))
def test_trace_bins_equal_the_integer_sums_at_every_lane_layout(d):
    """cpw = 128, 64, 2, 1, 1 rows side by side and two column tiles; bins of one generation, a ragged last bin, a bin wider than the
    window; a window that starts at generation 2"""
    H, X, _ = S.integer_history(S.TR_G, S.TR_N, d, seed=300 + d)
    e = _installed(H, X)
    try:
        for every in S.TR_EVERY:
            _check_traces(e, H, 0, S.TR_G, every)
            _check_traces(e, H, S.TR_G_LO, S.TR_G, every)
    finally:
        e.close()


@pytest.mark.parametrize("case", [S.TR_PARTS, S.TR_EMPTY], ids=["eight_parts", "an_empty_part"])
def test_trace_bins_cut_into_parts(case):
    """Bins cut into parts (tr_part) and folded in index order (tr_fold_kernel).

    Can a part be EMPTY on one rank?  Yes.  trace_parts sizes `parts` from the rows of a FULL bin (rows_grid: parts <= ceil(rows_per_bin /
    (4 * rows_per_sweep))), while tr_part cuts each bin's own rows into chunks of ceil(rows / parts):
      * the ragged last bin has fewer rows than that.  d = 255 (cpw = 1, 4 rows per sweep), N = 4, every = 9, 10 generations: 36 rows per
        bin give 3 parts; the last bin holds 4 rows, chunk = 2, and part 2 starts at row 4 = its end.  This is the second case here.
      * a full bin can do it too, since (parts - 1) * ceil(rows / parts) < rows does not follow from that bound: 289 rows per bin with 56
        bins x 2 column tiles give min(2048 / 112, ceil(289 / 16)) = 18 parts of 17 rows, and 17 * 17 = 289 leaves the 18th empty.  (That
        shape needs a history of 33 MB; the table asserts its arithmetic, and the empty part it produces is the one the small case runs:
        tr_part clamps lo and hi to the bin's end, the accumulator stays as tr_init left it, and tr_merge_moments skips n = 0.)
    So traces.h is right to say "the last ones may be empty", and an empty part must leave counts, shift, sums, min and max untouched."""
    H, X, _ = S.integer_history(case["G"], case["N"], case["d"], seed=case["N"])
    e = _installed(H, X)
    try:
        _check_traces(e, H, 0, case["G"], case["every"])
        _check_traces(e, H, 1, case["G"], case["every"])
    finally:
        e.close()
