"""What tests/test_stat_shapes_host.py and tests/test_gpu_stat_shapes.py share: the shapes at which the covariance, quantile, histogram,
trace and raw-moment kernels of the resident history change their path, the inputs on which every one of these statistics has an EXACT
reference, and the host launch arithmetic restated in Python, so that every case asserts the path it is there for.

EXACTNESS.  integer_history holds integers |x| <= 8 and an integer centre |c| <= 8, so |x - c| <= 16 and every product is an integer <= 256:
any partial sum that any order of additions, any merge of shifted accumulators (trace_acc.h: n d, 2 d S1, n d^2 with an integer d) and any
MFMA accumulation can form is an integer of magnitude <= rows * 256 < 2^53, which float64 holds exactly.  The device must therefore return
the integer sums bit for bit whatever its order -- a wrong lane, row, column, tile or tail cannot.  Quantiles and histogram counts are
NumPy's values as they stand.  Nothing here has a tolerance.

THE PATHS.  The constants are read from the kernel headers and sampler.hip, the launch rules are restated from the host code named next to
each function, and the tables carry what each case claims (T, tiles, blocks, trips round the loop, slots per tile, parts ...).  assert_*
recompute the claims: a later change of a constant or of a rule fails tests/test_stat_shapes_host.py on the CPU instead of silently moving a
case off its branch."""
import os
import re

import numpy as np

from bipymc_amd import quantiles as Q

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "bipymc_amd", "csrc")
_text = {}


def _const(source, name):
    """`constexpr <integer type> name = <integer expression>;` of a file under bipymc_amd/csrc"""
    if source not in _text:
        with open(os.path.join(CSRC, source)) as f:
            _text[source] = f.read()
    m = re.search(r"constexpr\s+(?:int|uint32_t|uint64_t)\s+%s\s*=\s*([^;]+);" % name, _text[source])
    assert m, (source, name)
    expr = re.sub(r"(?<=[0-9a-fA-F])u\b", "", m.group(1))
    assert re.match(r"^[0-9a-fA-Fx\s*+()-]+$", expr), expr
    return int(eval(expr, {"__builtins__": {}}))


COV_MAX_T, COV_BLK, COV_UNR = (_const("covariance.h", n) for n in ("COV_MAX_T", "COV_BLK", "COV_UNR"))
QS_THREADS, QS_SLOTS, QS_UNR = (_const("quantiles.h", n) for n in ("QS_THREADS", "QS_SLOTS", "QS_UNR"))
HS_THREADS, HS_UNR = (_const("histograms.h", n) for n in ("HS_THREADS", "HS_UNR"))
HS_LDS_TILE, HS_LDS_TOTAL, HS_LDS_PAIRS, HS_TILE_PAIRS = (_const("sampler.hip", n) for n in ("HS_LDS_TILE", "HS_LDS_TOTAL", "HS_LDS_PAIRS",
                                                                                             "HS_TILE_PAIRS"))
TR_THREADS, TR_UNR = (_const("traces.h", n) for n in ("TR_THREADS", "TR_UNR"))
MOM_THREADS = _const("kernels.h", "MOM_THREADS")


def _cdiv(a, b):
    return -(-a // b)


def ld_of(d):
    """rows are padded to an even number of doubles (16-byte rows: kernels.h, moments_partial_kernel)"""
    return d + (d & 1)


def rows_grid(rows, n_tiles, rows_per_sweep):
    """sampler.hip rows_grid: workgroups along the rows"""
    nby = max(1, 2048 // n_tiles)
    nby = min(nby, _cdiv(rows, 4 * rows_per_sweep))
    return max(nby, (rows >> 31) + 1)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def integer_history(G, N, d, seed):
    """-> (H (G, N, d) of integers in [-8, 8] as float64, drawn independently in every position; the state = the last row; an integer centre
    c (d,), |c_k| <= 8)"""
    rs = np.random.RandomState(seed)
    H = rs.randint(-8, 9, size=(G, N, d)).astype(np.float64)
    c = rs.randint(-8, 9, size=d).astype(np.float64)
    return H, H[-1].copy(), c


def _from_bits(b):
    return np.asarray(b, dtype=np.uint64).view(np.float64)


_ONE, _TWO, _MTHREE = (int(np.array([v]).view(np.uint64)[0]) for v in (1.0, 2.0, -3.0))
SPECIALS = np.array([np.inf, -np.inf, 1.7976931348623157e308, -1.7976931348623157e308, 2.2250738585072014e-308, -2.2250738585072014e-308, 0.0,
                     -0.0, 1.0, -1.0])
Q41 = np.linspace(0, 1, 41)


def quantile_history(G, N, seed):
    """-> (G, N, 6):
    0  1.0 + k ulp, k uniform in [0, 60000): every key shares its six leading bytes, passes 7 and 8 (bits = 48, 56) decide
    1  a ladder of denormals across zero, k * 5e-324 for k in [-300, 300], with both signed zeros
    2  2.0 +- k ulp: the keys straddle an exponent change
    3  draws from {+-inf, +-max, +-tiny, +-0.0, +-1}: NumPy's interpolation gives NaN where it meets inf - inf
    4  -3.0 - k ulp: negative keys, the flipped branch of qs_key
    5  standard normal: the column whose 41 quantiles follow more than QS_SLOTS prefixes"""
    rs = np.random.RandomState(seed)
    n = G * N
    H = np.empty((n, 6))
    H[:, 0] = _from_bits(np.uint64(_ONE) + rs.randint(0, 60000, size=n).astype(np.uint64))
    k = rs.randint(-300, 301, size=n)
    H[:, 1] = k * 5e-324
    zero = np.nonzero(k == 0)[0]
    H[zero, 1] = np.where(rs.randint(0, 2, size=len(zero)) == 1, -0.0, 0.0)
    H[[3, n - 2], 1] = -0.0                                   # (both signs whatever was drawn, the second inside the two-row window)
    H[[5, n - 1], 1] = 0.0
    H[:, 2] = _from_bits((_TWO + rs.randint(-2000, 2001, size=n)).astype(np.uint64))
    H[:, 3] = SPECIALS[rs.randint(0, len(SPECIALS), size=n)]
    H[:, 4] = _from_bits(np.uint64(_MTHREE) + rs.randint(0, 60000, size=n).astype(np.uint64))
    H[:, 5] = rs.normal(size=n)
    return H.reshape(G, N, 6)


def shifted_normal_history(G, N, d, seed):
    """column 5 of quantile_history(G, N, seed) repeated and shifted by the column index"""
    col = quantile_history(G, N, seed)[:, :, 5]
    return col[:, :, None] + np.arange(d, dtype=np.float64)


# ---- covariance (sampler.hip bpm_reduce_cov; covariance.h) -------------------------------------------------------------------------------
def cov_plan(dim, rows):
    """bpm_reduce_cov's launch: `T = n_tiles <= COV_MAX_T ? n_tiles : COV_BLK`, `n_blk`, `n_off`, the `nbx` rule; trips = how often
    workgroup 0 goes round cov_partial_kernel's double-buffered loop (`g += step * COV_UNR`)"""
    n_tiles = _cdiv(dim, 16)
    T = n_tiles if n_tiles <= COV_MAX_T else COV_BLK
    n_blk = _cdiv(n_tiles, T)
    n_off = n_blk * (n_blk - 1) // 2
    n_grp = _cdiv(rows, 4)
    want = 1024 if T > COV_BLK else 2048
    nbx = max(1, min(want // max(n_blk, n_off, 1), _cdiv(n_grp, COV_UNR)))
    return dict(T=T, n_tiles=n_tiles, n_blk=n_blk, n_off=n_off, nbx=nbx, n_grp=n_grp, trips=_cdiv(n_grp, nbx * COV_UNR),
                last_cols=dim - 16 * (n_tiles - 1), last_blk_tiles=n_tiles - T * (n_blk - 1))


COV_N, COV_G = 8, 5
COV_BURNS = (0, 3, 17, 35, 38)          # windows of 40, 37, 23, 5 and 2 rows; r_lo = 3, 17, 35 is no multiple of 4
# dim: (T, columns of the last tile) -- cov_partial_kernel<T, true>, T = 1 ... 7, each with a full last tile and with one of a single column
COV_SINGLE = {1: (1, 1), 15: (1, 15), 17: (2, 1), 32: (2, 16), 33: (3, 1), 48: (3, 16), 49: (4, 1), 64: (4, 16), 65: (5, 1), 80: (5, 16),
              81: (6, 1), 96: (6, 16), 97: (7, 1), 112: (7, 16)}
# dim: (tiles, blocks of COV_BLK tiles, block pairs = launches of cov_partial_kernel<COV_BLK, false>, tiles of the last block, columns of the
# last tile) -- 129: a third block of one tile of one column; 193: cov_block_pair decodes pairs of more than one row (bi = 0, 1, 2)
COV_BLOCKED = {113: (8, 2, 1, 4, 1), 128: (8, 2, 1, 4, 16), 129: (9, 3, 3, 1, 1), 193: (13, 4, 6, 1, 1)}
# (dim, N, G, n_burn): (T, nbx, trips) -- ceil(rows / 4) > COV_UNR * nbx: a second, ragged trip round the double-buffered loop
COV_LONG = {(193, 8, 700, 3): (4, 341, 2), (112, 16, 1030, 5): (7, 1024, 2), (40, 32, 1030, 1): (3, 2048, 2)}


def assert_cov_paths():
    for dim, (T, last) in COV_SINGLE.items():
        p = cov_plan(dim, COV_N * COV_G)
        assert (p["T"], p["last_cols"], p["n_blk"], p["n_off"]) == (T, last, 1, 0), (dim, p)
    assert sorted(set(T for T, _ in COV_SINGLE.values())) == list(range(1, COV_MAX_T + 1))
    for T in range(1, COV_MAX_T + 1):
        assert sorted(l for t, l in COV_SINGLE.values() if t == T) == [1, 16] or T == 1, T
    assert max(COV_SINGLE) == 16 * COV_MAX_T and min(COV_BLOCKED) == 16 * COV_MAX_T + 1
    for dim, (n_tiles, n_blk, n_off, last_blk, last) in COV_BLOCKED.items():
        p = cov_plan(dim, COV_N * COV_G)
        assert (p["T"], p["n_tiles"], p["n_blk"], p["n_off"], p["last_blk_tiles"], p["last_cols"]) == (COV_BLK, n_tiles, n_blk, n_off, last_blk,
                                                                                                  last), (dim, p)
    for n_burn in COV_BURNS:
        rows = COV_N * COV_G - n_burn
        assert rows >= 1 and cov_plan(193, rows)["trips"] == 1
    assert any(b % 4 for b in COV_BURNS) and min(COV_N * COV_G - b for b in COV_BURNS) == 2
    for (dim, N, G, n_burn), (T, nbx, trips) in COV_LONG.items():
        rows = N * G - n_burn
        p = cov_plan(dim, rows)
        assert (p["T"], p["nbx"], p["trips"]) == (T, nbx, trips) and trips > 1, (dim, p)
        assert p["n_grp"] % (p["nbx"] * COV_UNR) != 0 and rows % 4 != 0 and n_burn % 4 != 0      # a ragged last trip, a ragged last group
        assert N * G * dim * 8 <= 15 << 20


# ---- raw moments (sampler.hip bpm_reduce_moments; kernels.h moments_partial_kernel) ---------------------------------------------------------
def moments_plan(dim, rows):
    """`nb = min(2048, ceil(rows / 64))` blocks; ppp pairs per pass over the columns, passes over the columns, rpi rows per iteration"""
    pairs = ld_of(dim) // 2
    ppp = min(pairs, MOM_THREADS)
    return dict(nb=max(1, min(2048, _cdiv(rows, 64))), passes=_cdiv(pairs, ppp), rpi=MOM_THREADS // ppp, last_pass=pairs - ppp * (_cdiv(pairs, ppp) - 1))


MOM_N, MOM_G = 8, 9
MOM_BURNS = {0: 72, 7: 65, 30: 42}       # n_burn: rows -- two blocks of 36; 64 * 1 + 1 rows: two blocks of 33 and 32; fewer than 64: one block
# dim: (passes over the columns, pairs of the last pass, rows per iteration) -- 511 / 512: ld / 2 = 256 fills the block; 513: one pair left
MOM_DIMS = {1: (1, 1, 256), 2: (1, 1, 256), 3: (1, 2, 128), 511: (1, 256, 1), 512: (1, 256, 1), 513: (2, 1, 1)}


def assert_moments_paths():
    for dim, (passes, last, rpi) in MOM_DIMS.items():
        p = moments_plan(dim, MOM_N * MOM_G)
        assert (p["passes"], p["last_pass"], p["rpi"]) == (passes, last, rpi), (dim, p)
    for n_burn, rows in MOM_BURNS.items():
        assert MOM_N * MOM_G - n_burn == rows
    assert [moments_plan(3, r)["nb"] for r in MOM_BURNS.values()] == [2, 2, 1]
    assert any(r < 64 for r in MOM_BURNS.values()) and any(r % 64 == 1 for r in MOM_BURNS.values())


# ---- quantiles (sampler.hip bpm_quantile_histogram; quantiles.h) ---------------------------------------------------------------------------
def quantile_tiles(pk):
    """the tile loop of bpm_quantile_histogram over the sorted coordinates of the slots -> [(first slot, slots, first coordinate, coordinates)]"""
    pk = [int(k) for k in pk]
    tiles, j = [], 0
    while j < len(pk):
        j0, k0 = j, pk[j]
        while j < len(pk) and j - j0 < QS_SLOTS and pk[j] - k0 < QS_SLOTS:
            j += 1
        tiles.append((j0, j - j0, k0, pk[j - 1] - k0 + 1))
    return tiles


def quantile_grid(pk, rows):
    """-> (tiles, cpw, nby): `kw_min` over the tiles, `cpw = QS_THREADS / kw_min`, rows_grid(rows, n_tiles, QS_UNR * cpw)"""
    tiles = quantile_tiles(pk)
    cpw = QS_THREADS // min(t[3] for t in tiles)
    return tiles, cpw, rows_grid(rows, len(tiles), QS_UNR * cpw)


def starts_inside_a_coordinate(pk, tiles):
    """a tile whose first slot continues the coordinate of the slot before it"""
    return any(j0 > 0 and int(pk[j0]) == int(pk[j0 - 1]) for j0, _, _, _ in tiles)


QH_G, QH_N, QH_SEED = 40, 64, 17
QH_BURNS = (0, 7, 64 * 39, 64 * 40 - 2, 64 * 40 - 1)        # the last two windows hold 2 rows and 1 row
Q_SPAN_DIMS = (1, 2, 31, 32, 33, 64, 65)                    # one quantile: a slot per coordinate in pass 0, cut by the 32-coordinate span
Q_SPAN_TILES = {1: [1], 2: [2], 31: [31], 32: [32], 33: [32, 1], 64: [32, 32], 65: [32, 32, 1]}      # d: coordinates per tile in pass 0
# rows_grid's step from one workgroup along the rows to two: d = 2 (kw = 2, cpw = 128), rows = 4 * QS_UNR * cpw and one more
Q_ROWS_N, Q_ROWS_G = 4, 513
Q_ROWS_BURNS = {4: (2048, 1), 3: (2049, 2)}                 # n_burn: (rows, nby)


def direct_slot_cases():
    """Hand-built requests for bpm_quantile_histogram -> [(name, history, n_burn, pk, pv, bits, (tiles, a tile starts inside a coordinate))]"""
    H = quantile_history(QH_G, QH_N, QH_SEED)
    K = Q.to_key(H.reshape(-1, 6))
    W = shifted_normal_history(6, 8, 65, QH_SEED)
    p16 = np.unique(K[:, 5] >> np.uint64(48))                # the 16-bit prefixes that occur in the normal column
    assert len(p16) >= 65
    k0 = np.unique(K[:, 0])[:30]                             # the 30 smallest distinct keys of column 0
    p56 = np.unique(k0 >> np.uint64(8))
    assert not np.any((K[:, 5] >> np.uint64(56)) == 0)       # no key of the normal column starts with the byte 0
    z = np.uint64(0)
    cases = [
        ("one slot", H, 0, [5], [z], 0, (1, False)),
        ("33 slots on one coordinate", H, 7, [5] * 33, p16[:33], 16, (2, True)),
        ("65 slots on one coordinate", H, 7, [5] * 65, p16[:65], 16, (3, True)),
        ("coordinates 0 and 31: one tile of the full span", W, 0, [0, 31], [z, z], 0, (1, False)),
        ("coordinates 0 and 32: the span cuts", W, 0, [0, 32], [z, z], 0, (2, False)),
        ("coordinates 0, 31, 32, 63, 64", W, 5, [0, 31, 32, 63, 64], [z] * 5, 0, (3, False)),
        ("a prefix no key carries", H, 0, [5], [z], 8, (1, False)),
        ("the last byte of column 0", H, 0, [0] * len(p56), p56, 56, (1, False)),
        # 20 + 20 + 3 slots: the second tile starts at the 13th slot of coordinate 1 and goes on to coordinate 5 (the leading bytes asked for
        # include the ones that occur: 0xBF of 1.0, 0x7F / 0x80 either side of zero, 0x40 / 0xBF of the normal column)
        ("a tile that starts inside coordinate 1", H, 7, [0] * 20 + [1] * 20 + [5] * 3,
         list(range(0xAC, 0xC0)) + list(range(0x70, 0x84)) + [0x40, 0xBF, 0xC0], 8, (2, True)),
    ]
    return [(name, Hc, n_burn, np.asarray(pk, dtype=np.int32), np.asarray(pv, dtype=np.uint64), bits, claim)
            for name, Hc, n_burn, pk, pv, bits, claim in cases]


def assert_quantile_paths():
    for name, Hc, n_burn, pk, pv, bits, (n_tiles, inside) in direct_slot_cases():
        tiles = quantile_tiles(pk)
        assert len(tiles) == n_tiles and starts_inside_a_coordinate(pk, tiles) == inside, (name, tiles)
        assert all(ns <= QS_SLOTS and kw <= QS_SLOTS for _, ns, _, kw in tiles)
        pv = np.asarray(pv, dtype=np.uint64)
        assert all(int(v) >> bits == 0 for v in pv) if bits else not pv.any()
        key = list(zip(pk, [int(v) for v in pv]))
        assert key == sorted(set(key)), name                 # the ABI's order: by coordinate, prefixes of a coordinate strictly increasing
    for d, per_tile in Q_SPAN_TILES.items():
        assert [t[3] for t in quantile_tiles(range(d))] == per_tile, d
    assert sorted(Q_SPAN_TILES) == list(Q_SPAN_DIMS) and QS_SLOTS in Q_SPAN_DIMS and QS_SLOTS + 1 in Q_SPAN_DIMS
    for n_burn, (rows, nby) in Q_ROWS_BURNS.items():
        assert Q_ROWS_N * Q_ROWS_G - n_burn == rows
        tiles, cpw, got = quantile_grid([0, 1], rows)
        assert (len(tiles), cpw, got) == (1, QS_THREADS // 2, nby), (rows, cpw, got)
    assert sorted(r for r, _ in Q_ROWS_BURNS.values()) == [4 * QS_UNR * (QS_THREADS // 2), 4 * QS_UNR * (QS_THREADS // 2) + 1]
    assert [QH_G * QH_N - b for b in QH_BURNS][-2:] == [2, 1]


# ---- histograms (sampler.hip bpm_hist_range / bpm_hist_marginals / bpm_hist_pairs; histograms.h) ----------------------------------------------
def pair_tiles(pa, pb, bins2d):
    """bpm_hist_pairs: `tp_max`, equal shares of `tp` pairs, each tile's distinct slots in order of first use
    -> (tp_max, [(first pair, pairs, [slots])])"""
    cells = bins2d * bins2d
    tp_max = max(1, min(HS_TILE_PAIRS, HS_LDS_PAIRS // (cells * 4)))
    P = len(pa)
    n_tiles = _cdiv(P, tp_max)
    tp = _cdiv(P, n_tiles)
    tiles = []
    for p0 in range(0, P, tp):
        n = min(tp, P - p0)
        slots = []
        for p in range(p0, p0 + n):
            for s in (int(pa[p]), int(pb[p])):
                if s not in slots:
                    slots.append(s)
        tiles.append((p0, n, slots))
    return tp_max, tiles


def marginal_plan(m, bins):
    """bpm_hist_marginals: `kw` slots per tile, the tiles, `rep` copies of the counts -> (kw, slots of the last tile, tiles, rep)"""
    slot_bytes = bins * 4 + (bins + 1) * 8
    kw = max(1, min(m, HS_THREADS, HS_LDS_TILE // slot_bytes))
    n_tiles, cpw = _cdiv(m, kw), HS_THREADS // kw
    rep = max(1, min(8, cpw, (HS_LDS_TOTAL - kw * (bins + 1) * 8) // (kw * bins * 4)))
    return kw, m - kw * (n_tiles - 1), n_tiles, rep


def range_plan(d):
    """bpm_hist_range (and tr_bins_kernel: the same lane layout) -> (kw, column tiles, cpw, busy lanes of the last tile)"""
    ld = ld_of(d)
    kw = min(ld, HS_THREADS)
    n_tiles = _cdiv(ld, kw)
    return kw, n_tiles, HS_THREADS // kw, ld - kw * (n_tiles - 1)


HP_WIDE = dict(d=130, N=8, G=30, bins2d=8, pairs=[(2 * i, 2 * i + 1) for i in range(64)])
HP_WIDE_ROWS = (240, 1, 7, 8, 9)         # the whole window; one row; rc - 1, rc and rc + 1 rows (rc = cpw1 * HS_UNR = 8)
HP_ALL = dict(d=24, N=8, G=30)
HP_ALL_BINS = {5: (64, 5, 56, 52), 11: (64, 5, 56, 52), 12: (56, 5, 56, 52), 46: (3, 92, 3, 3), 64: (2, 138, 2, 2)}   # bins2d: (tp_max, tiles, tp, last tile)
HP_ODD_PAIRS = {"a coordinate paired with itself": [(3, 3), (0, 1), (5, 5)], "the same pair twice": [(0, 1), (2, 4), (0, 1), (4, 2)]}
HM_CASES = {(200, 20): (165, 35, 2), (7, 1024): (3, 1, 3)}        # (m, bins): (kw, slots of the last tile, tiles)
HR_DIMS = {255: (256, 1, 1, 256), 257: (256, 2, 1, 2)}            # d: (kw, column tiles, cpw, busy lanes of the last tile)


def all_pairs(m):
    return [(a, b) for a in range(m) for b in range(a + 1, m)]


def assert_histogram_paths():
    pa, pb = zip(*HP_WIDE["pairs"])
    tp_max, tiles = pair_tiles(pa, pb, HP_WIDE["bins2d"])
    assert tp_max == HS_TILE_PAIRS == 64 and len(tiles) == 1 and tiles[0][1] == 64 and len(tiles[0][2]) == 128
    cpw1 = HS_THREADS // 128
    assert cpw1 == 2 and cpw1 * HS_UNR == 8
    assert HP_WIDE_ROWS == (HP_WIDE["N"] * HP_WIDE["G"], 1, cpw1 * HS_UNR - 1, cpw1 * HS_UNR, cpw1 * HS_UNR + 1)
    pa, pb = zip(*all_pairs(HP_ALL["d"]))
    assert len(pa) == 276
    for bins2d, (tp_max, n_tiles, tp, last) in HP_ALL_BINS.items():
        got_max, tiles = pair_tiles(pa, pb, bins2d)
        assert (got_max, len(tiles), tiles[0][1], tiles[-1][1]) == (tp_max, n_tiles, tp, last), (bins2d, got_max, len(tiles))
        listed = [s for _, _, slots in tiles for s in slots]
        assert max(listed.count(s) for s in set(listed)) > 1                 # a slot re-listed in a later tile
    assert HS_LDS_PAIRS // (11 * 11 * 4) >= HS_TILE_PAIRS > HS_LDS_PAIRS // (12 * 12 * 4)      # bins2d <= 11: the pair limit binds, not the LDS
    for (m, bins), (kw, last, n_tiles) in HM_CASES.items():
        assert marginal_plan(m, bins)[:3] == (kw, last, n_tiles), (m, bins, marginal_plan(m, bins))
    for d, plan in HR_DIMS.items():
        assert range_plan(d) == plan, (d, range_plan(d))


# ---- traces (sampler.hip bpm_trace_bins, trace_parts; traces.h tr_part) ---------------------------------------------------------------------
def trace_plan(d, N, g_lo, g_hi, every):
    """-> dict(T bins, rows of every bin, kw, column tiles, cpw, parts, per bin the rows of every part as tr_part cuts them)"""
    span = g_hi - g_lo
    ev = min(every, span)
    T = _cdiv(span, ev)
    kw, n_tiles, cpw, _ = range_plan(d)
    parts = rows_grid(ev * N, T * n_tiles, cpw * TR_UNR)
    rows = [(min(g_lo + (t + 1) * ev, g_hi) - (g_lo + t * ev)) * N for t in range(T)]
    cut = []
    for r in rows:
        chunk = _cdiv(r, parts)
        cut.append([max(0, min(r, (p + 1) * chunk) - min(r, p * chunk)) for p in range(parts)])
    return dict(T=T, rows=rows, kw=kw, n_tiles=n_tiles, cpw=cpw, parts=parts, cut=cut)


TR_N, TR_G = 5, 7
TR_DIMS = {1: (128, 1), 3: (64, 1), 127: (2, 1), 129: (1, 1), 255: (1, 1), 257: (1, 2)}       # d: (cpw, column tiles)
TR_EVERY = {1: [5] * 7, 3: [15, 15, 5], 12: [35]}            # every: rows of the bins of [0, 7) -- a ragged last bin; a bin wider than the window
TR_G_LO = 2
TR_PARTS = dict(d=255, N=40, G=7, every=3)                   # rows_per_bin = 120: 8 parts of 15 rows; the last bin (40 rows): 8 parts of 5
TR_EMPTY = dict(d=255, N=4, G=10, every=9)                   # 36 rows per bin: 3 parts; the last bin holds 4 rows: parts of 2, 2 and 0 rows


def assert_trace_paths():
    for d, (cpw, n_tiles) in TR_DIMS.items():
        for every, rows in TR_EVERY.items():
            p = trace_plan(d, TR_N, 0, TR_G, every)
            assert (p["cpw"], p["n_tiles"], p["rows"]) == (cpw, n_tiles, rows), (d, every, p)
            assert all(sum(c) == r and 0 not in c for c, r in zip(p["cut"], rows))
        assert trace_plan(d, TR_N, TR_G_LO, TR_G, 3)["rows"] == [15, 10]
    assert trace_plan(255, TR_N, 0, TR_G, 12)["cut"] == [[12, 12, 11]]        # cpw = 1: the 35 rows of the one wide bin in three parts
    p = trace_plan(TR_PARTS["d"], TR_PARTS["N"], 0, TR_PARTS["G"], TR_PARTS["every"])
    assert p["rows"] == [120, 120, 40] and p["parts"] == 8 and p["cut"] == [[15] * 8, [15] * 8, [5] * 8], p
    p = trace_plan(TR_EMPTY["d"], TR_EMPTY["N"], 0, TR_EMPTY["G"], TR_EMPTY["every"])
    assert p["rows"] == [36, 4] and p["parts"] == 3 and p["cut"] == [[12, 12, 12], [2, 2, 0]], p
    # a FULL bin can leave parts empty as well: 56 bins x 2 column tiles, 289 rows per bin -> 18 parts of 17 rows, 17 * 17 = 289
    assert rows_grid(289, 56 * 2, 1 * TR_UNR) == 18 and _cdiv(289, 18) * 17 >= 289
