"""Exact quantiles of a sampler's resident history: what `np.quantile(param_est(n_burn)[2], q, axis=0)` returns, computed without moving
the history off the GPU(s).

The device counts (bpm_quantile_begin / bpm_quantile_histogram, bipymc_amd/csrc/quantiles.h); this module runs an MSD radix select with
8-bit digits over order-preserving 64-bit keys of the doubles, 8 passes.  In each pass every rank counts, for every (coordinate, prefix) the
select still follows, the keys of its window under that prefix by their next digit; the parts travel through `allgather`, and every rank
adds them and picks the next digit of every target with the same integer arithmetic in the same order, so every rank returns the same bits.
After the 8th pass the prefixes are the keys of the order statistics NumPy's linear method reads, and NumPy's interpolation is restated on
them.

NumPy's default method ("linear", numpy/lib/_function_base_impl.py, NumPy 2.2):
  virtual index v = (n - 1) * q;  previous = floor(v), next = previous + 1; where v >= n - 1 both are -1 (the last), where v < 0 both 0;
  gamma = v - previous (against the clamped previous index);  _lerp: a + (b - a) * gamma, or b - (b - a) * (1 - gamma) where gamma >= 0.5;
  a column that holds a NaN gives NaN.  An integer q (0 or 1) takes the order statistic itself.
"""
from __future__ import division

import numpy as np

from ._history_stats import check_n_burn, empty_window
from .comm import single_process_allgather  # noqa: F401  (for callers without a communicator)

DEFAULT_Q = (0.05, 0.5, 0.95)
DIGIT_BITS = 8
PASSES = 64 // DIGIT_BITS
NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
_SIGN = np.uint64(1 << 63)


def to_key(x):
    """float64 array -> uint64 keys in the same order: negative -> all bits flipped, otherwise the sign bit set; every NaN -> NAN_KEY"""
    x = np.asarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    k = np.where(b & _SIGN, ~b, b | _SIGN)
    return np.where(np.isnan(x), NAN_KEY, k).astype(np.uint64)


def from_key(k):
    """the inverse of to_key (NAN_KEY -> a NaN)"""
    k = np.asarray(k, dtype=np.uint64)
    b = np.where(k & _SIGN, k & ~_SIGN, ~k).astype(np.uint64)
    return b.view(np.float64)


def check_q(q):
    """q as NumPy takes it (a Python scalar in float64), validated with NumPy's message"""
    if isinstance(q, (int, float)) and not isinstance(q, bool):
        q = np.asanyarray(q, dtype=np.float64)
    else:
        q = np.asanyarray(q)
    if q.dtype.kind not in "iuf":
        raise ValueError("Quantiles must be in the range [0, 1]")
    if not (np.all(q >= 0) and np.all(q <= 1)):
        raise ValueError("Quantiles must be in the range [0, 1]")
    return q


def targets(n, q):
    """-> (previous, next, gamma) for a window of n values: 0-based order statistics (arrays shaped like q, int64) and the interpolation
    weight (None for an integer q, which takes previous itself)"""
    n = int(n)
    v = np.asanyarray((n - 1) * q)
    if np.issubdtype(v.dtype, np.integer):
        idx = np.array(v, dtype=np.int64)
        return idx, idx.copy(), None
    prev = np.asanyarray(np.floor(v))
    nxt = np.asanyarray(prev + 1)
    above = v >= n - 1
    prev = np.where(above, -1, prev)
    nxt = np.where(above, -1, nxt)
    below = v < 0
    prev = np.where(below, 0, prev)
    nxt = np.where(below, 0, nxt)
    prev_i = np.asarray(prev).astype(np.intp)
    nxt_i = np.asarray(nxt).astype(np.intp)
    gamma = np.asanyarray(np.asanyarray(v - prev_i), dtype=v.dtype)
    return np.where(prev_i < 0, prev_i + n, prev_i).astype(np.int64), np.where(nxt_i < 0, nxt_i + n, nxt_i).astype(np.int64), gamma


def lerp(a, b, t):
    """NumPy's _lerp: a, b (len(q), dim), t (len(q), 1)"""
    diff_b_a = np.subtract(b, a)
    out = np.asanyarray(np.add(a, diff_b_a * t))
    np.subtract(b, diff_b_a * (1 - t), out=out, where=t >= 0.5, casting="unsafe", dtype=type(out.dtype))
    return out


def finish(n, q, order_stats, has_nan):
    """order_stats(ranks) -> (len(ranks), dim) values of those 0-based order statistics; has_nan: (dim,) bool -> np.quantile's result"""
    prev, nxt, gamma = targets(n, q)
    p = prev.reshape(-1)
    x = nxt.reshape(-1)
    a = order_stats(p)
    if gamma is None:
        res = np.array(a, dtype=np.float64)
    else:
        b = order_stats(x)
        res = lerp(a, b, gamma.reshape(-1, 1))
    res = np.array(res, dtype=np.float64)
    res[:, np.asarray(has_nan, dtype=bool)] = np.nan
    return res.reshape(tuple(q.shape) + (res.shape[1],))


def select(histogram, allgather, n, ranks, dim):
    """The collective MSD radix select: for each coordinate k < dim and each 0-based rank in `ranks` (sorted, distinct, < n), the key of the
    rank-th smallest value.  histogram(prefix_dim, prefixes, bits) -> (hist (n_prefix, 256) int, n_nan (n_prefix,) int): this rank's counts
    (HipEngine.quantile_histogram).  -> (keys (len(ranks), dim) uint64, n_nan (dim,) int64)"""
    ranks = np.asarray(ranks, dtype=np.int64)
    nr = len(ranks)
    pre = np.zeros((dim, nr), dtype=np.uint64)              # prefix followed by each target
    rem = np.tile(ranks, (dim, 1))                          # its rank among the keys under that prefix
    n_nan = None
    for p in range(PASSES):
        bits = DIGIT_BITS * p
        kk = np.repeat(np.arange(dim, dtype=np.int64), nr)
        flat = pre.reshape(-1)
        # the distinct (coordinate, prefix) slots, sorted by coordinate then prefix: targets that share a prefix share a histogram
        slots, inv = np.unique(np.stack([kk.astype(np.uint64), flat], axis=1), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        parts = allgather(histogram(slots[:, 0].astype(np.int32), slots[:, 1].astype(np.uint64), bits))
        hist = np.zeros((len(slots), 256), dtype=np.int64)
        nn = np.zeros(len(slots), dtype=np.int64)
        for h, c in parts:
            hist += np.asarray(h, dtype=np.int64).reshape(len(slots), 256)
            nn += np.asarray(c, dtype=np.int64).reshape(len(slots))
        if p == 0:
            n_nan = nn                                      # one slot per coordinate, in coordinate order
        cum = np.cumsum(hist, axis=1)
        r = rem.reshape(-1)
        c = cum[inv]
        digit = np.sum(c <= r[:, None], axis=1)             # the bin whose cumulative count first exceeds the rank
        if np.any(digit > 255):
            raise RuntimeError("quantiles: the histograms hold fewer keys than the window (the history changed between passes?)")
        below = np.where(digit > 0, np.take_along_axis(c, np.maximum(digit - 1, 0)[:, None], axis=1)[:, 0], 0)
        rem = (r - below).reshape(dim, nr)
        pre = ((flat << np.uint64(DIGIT_BITS)) | digit.astype(np.uint64)).reshape(dim, nr)
    return pre.T.copy(), n_nan


def compute(begin, histogram, allgather, n_burn, q=DEFAULT_Q, dim=None):
    """The collective driver.  begin(n_burn) -> this rank's row count in the window (HipEngine.quantile_begin); histogram: see select();
    allgather(obj) -> [obj of every rank] in rank order ([obj] for one process, single_process_allgather).  -> np.quantile's result,
    shape q.shape + (dim,)"""
    q = check_q(q)
    n_burn = check_n_burn("param_est_quantiles", n_burn)
    n = int(np.sum(np.asarray(allgather(begin(n_burn)), dtype=np.int64)))
    if n == 0:
        raise empty_window("param_est_quantiles", n_burn)
    prev, nxt, _ = targets(n, q)
    ranks = np.unique(np.concatenate([prev.reshape(-1), nxt.reshape(-1)]))
    keys, n_nan = select(histogram, allgather, n, ranks, int(dim))
    vals = from_key(keys)
    pos = {int(r): i for i, r in enumerate(ranks)}
    return finish(n, q, lambda rr: vals[[pos[int(r)] for r in rr]], n_nan > 0)
