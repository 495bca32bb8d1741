"""Marginal and pairwise histograms of a sampler's resident history: the counts behind a corner plot (the reference draws
`corner.corner(samples)`, mc_plot/mc_plot.py:16-29: a 1-D histogram per parameter, a 2-D histogram per pair), computed without moving the
history off the GPU(s).  The 1-D counts equal `np.histogram(col, bins, range)[0]`, the 2-D counts `np.histogram2d(col_a, col_b, bins2d,
range=[ra, rb])[0]`, exactly: counts are integers, so ranks merge by addition and the order of the additions does not matter.

The device finds the range and counts (bpm_hist_range / bpm_hist_marginals / bpm_hist_pairs, bipymc_amd/csrc/histograms.h); this module
restates NumPy's rules (NumPy 2.2, numpy/lib/_histograms_impl.py) around them:
  range    None: per coordinate (min, max) of the window, a ValueError "autodetected range of [..] is not finite" where the column holds a
           NaN or an infinity; a given range must be finite ("supplied range of [..] is not finite") and have lo <= hi ("max must be larger
           than min in range parameter."); lo == hi becomes (lo - 0.5, hi + 0.5);
  edges    np.linspace(lo, hi, bins + 1), bit for bit np.histogram_bin_edges (a range too narrow for that many distinct edges is its
           ValueError "Too many bins for data range"); the device receives the edges, never lo, hi or a width;
  binning  bin i counts edges[i] <= x < edges[i + 1], the last bin also x == edges[-1]; values outside the range and NaN count nowhere.
Every rank computes the same merged range, hence the same edges; the counts of the ranks travel through `allgather` and are added.
"""
from __future__ import division

import collections

import numpy as np

from ._history_stats import check_n_burn, empty_window
from .comm import single_process_allgather  # noqa: F401  (for callers without a communicator)

MAX_BINS = 1024
MAX_BINS2D = 64


class PosteriorHistograms(collections.namedtuple("PosteriorHistograms", ["dims", "edges", "counts", "pairs", "edges2d", "counts2d", "n"])):
    """dims (m,) coordinates; edges (m, bins + 1) float64; counts (m, bins) int64; pairs (P, 2) coordinates; edges2d (m, bins2d + 1);
    counts2d (P, bins2d, bins2d) int64, [pair, bin of a, bin of b]; n rows of the window, summed over ranks"""
    __slots__ = ()

    def density(self):
        """the 1-D counts as np.histogram(..., density=True) normalises them, counts / (counts.sum() * np.diff(edges)), in NumPy's own order
        of operations (counts / np.diff(edges) / counts.sum()) so that the bits are NumPy's; a row of all zeros gives NaN, as NumPy does"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.counts / np.diff(self.edges, axis=1) / self.counts.sum(axis=1, keepdims=True)


def check_bins(bins, limit, name):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)):
        raise TypeError("param_est_hist: %s must be an integer (got %r)" % (name, bins))
    if not 1 <= int(bins) <= limit:
        raise ValueError("param_est_hist: %s = %d is outside the supported 1 ... %d" % (name, int(bins), limit))
    return int(bins)


def check_dims(dims, dim):
    """-> (m,) int64 coordinates: all of them for None, else distinct indices in [0, dim) in the order given"""
    if dims is None:
        return np.arange(dim, dtype=np.int64)
    d = np.asarray(dims)
    if d.ndim != 1 or d.size == 0 or d.dtype.kind not in "iu":
        raise ValueError("param_est_hist: dims must be a non-empty sequence of coordinate indices")
    d = d.astype(np.int64)
    if d.min() < 0 or d.max() >= dim:
        raise ValueError("param_est_hist: dims must lie in [0, %d)" % dim)
    if len(np.unique(d)) != len(d):
        raise ValueError("param_est_hist: dims must be distinct")
    return d


def check_pairs(pairs, dims):
    """-> (P, 2) int64 coordinates: none for None, every a < b of dims (positions in dims, lexicographic) for "all", else the pairs given"""
    if pairs is None:
        return np.zeros((0, 2), dtype=np.int64)
    if isinstance(pairs, str):
        if pairs != "all":
            raise ValueError("param_est_hist: pairs must be None, \"all\" or a sequence of (a, b)")
        m = len(dims)
        return np.array([(dims[i], dims[j]) for i in range(m) for j in range(i + 1, m)], dtype=np.int64).reshape(-1, 2)
    p = np.asarray(pairs)
    if p.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu":
        raise ValueError("param_est_hist: pairs must be None, \"all\" or a sequence of (a, b) coordinate indices")
    p = p.astype(np.int64)
    if not np.all(np.isin(p, dims)):
        raise ValueError("param_est_hist: both members of every pair must be in dims")
    return p


def resolve_range(rng, m, lo, hi, n_nan, n_inf):
    """NumPy's _get_outer_edges for m coordinates.  rng: None, (lo, hi) for all, or (m, 2); lo, hi, n_nan, n_inf: (m,) of the window (lo and
    hi over the values that are not NaN).  -> (m, 2) float64"""
    if rng is None:
        out = np.empty((m, 2))
        for j in range(m):
            a, b = (np.nan, np.nan) if n_nan[j] > 0 else (lo[j], hi[j])
            if n_nan[j] > 0 or n_inf[j] > 0 or not (np.isfinite(a) and np.isfinite(b)):
                raise ValueError("autodetected range of [{}, {}] is not finite".format(a, b))
            out[j] = (a, b)
    else:
        r = np.asarray(rng, dtype=np.float64)
        if r.shape == (2,):
            r = np.tile(r, (m, 1))
        if r.shape != (m, 2):
            raise ValueError("param_est_hist: range must be None, (lo, hi) or an array of shape (%d, 2)" % m)
        out = r.copy()
        for a, b in out:
            if a > b:
                raise ValueError("max must be larger than min in range parameter.")
            if not (np.isfinite(a) and np.isfinite(b)):
                raise ValueError("supplied range of [{}, {}] is not finite".format(a, b))
    same = out[:, 0] == out[:, 1]
    out[same, 0] -= 0.5
    out[same, 1] += 0.5
    return out


def make_edges(ranges, bins, strict=True):
    """(m, 2) -> (m, bins + 1): np.linspace(lo, hi, bins + 1) per coordinate (np.histogram_bin_edges' uniform bins); as there, a range too
    narrow for `bins` distinct edges is a ValueError"""
    e = np.stack([np.linspace(a, b, bins + 1, endpoint=True, dtype=np.float64) for a, b in ranges])
    if strict and np.any(e[:, :-1] >= e[:, 1:]):
        raise ValueError("Too many bins for data range. Cannot create {} finite-sized bins.".format(bins))
    return e


def compute(hist_range, hist_marginals, hist_pairs, allgather, n_burn, dim, bins=20, range=None, dims=None, pairs=None, bins2d=None):
    """The collective driver.  hist_range(n_burn) -> (count, lo, hi, n_nan, n_inf) of this rank's rows (HipEngine.hist_range); hist_marginals(
    dims, edges) -> (m, bins) counts; hist_pairs(dims, edges2d, pair_a, pair_b) -> (P, bins2d, bins2d) counts (pair_a / pair_b are positions
    in dims); allgather(obj) -> [obj of every rank] in rank order ([obj] for one process, single_process_allgather).
    -> PosteriorHistograms, the same bits on every rank"""
    n_burn = check_n_burn("param_est_hist", n_burn)
    dim = int(dim)
    bins = check_bins(bins, MAX_BINS, "bins")
    dm = check_dims(dims, dim)
    pr = check_pairs(pairs, dm)
    # (bins2d defaults to bins; its own limit applies once it is given or a pair is asked for)
    bins2d = check_bins(bins if bins2d is None else bins2d, MAX_BINS2D if (bins2d is not None or len(pr)) else MAX_BINS, "bins2d")
    m = len(dm)
    parts = allgather(hist_range(n_burn))
    n = sum(int(p[0]) for p in parts)
    if n == 0:
        raise empty_window("param_est_hist", n_burn)
    lo = np.min([np.asarray(p[1], dtype=np.float64).reshape(dim) for p in parts], axis=0)[dm]
    hi = np.max([np.asarray(p[2], dtype=np.float64).reshape(dim) for p in parts], axis=0)[dm]
    n_nan = np.sum([np.asarray(p[3], dtype=np.int64).reshape(dim) for p in parts], axis=0)[dm]
    n_inf = np.sum([np.asarray(p[4], dtype=np.int64).reshape(dim) for p in parts], axis=0)[dm]
    ranges = resolve_range(range, m, lo, hi, n_nan, n_inf)
    edges = make_edges(ranges, bins)
    edges2d = edges if bins2d == bins else make_edges(ranges, bins2d, strict=len(pr) > 0)
    counts = np.zeros((m, bins), dtype=np.int64)
    for c in allgather(hist_marginals(dm, edges)):
        counts += np.asarray(c, dtype=np.int64).reshape(m, bins)
    counts2d = np.zeros((len(pr), bins2d, bins2d), dtype=np.int64)
    if len(pr):
        pos = {int(k): j for j, k in enumerate(dm)}
        pa = np.array([pos[int(a)] for a in pr[:, 0]], dtype=np.int32)
        pb = np.array([pos[int(b)] for b in pr[:, 1]], dtype=np.int32)
        for c in allgather(hist_pairs(dm, edges2d, pa, pb)):
            counts2d += np.asarray(c, dtype=np.int64).reshape(len(pr), bins2d, bins2d)
    return PosteriorHistograms(dm, edges, counts, pr, edges2d, counts2d, n)
