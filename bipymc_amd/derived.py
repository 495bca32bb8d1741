"""Posterior summaries of user-written derived quantities, computed where the history lives.

Every fitting script of the reference ends by taking `param_est(n_burn)[2]` to the host and running a function over the samples: a ratio of two
parameters with its mean and standard deviation (examples/ex_exp_fit.py:197-202), the fitted model at every sample for the trajectory picture
(examples/ex_exp_fit.py:176-192; ex_line_fit.py and ex_para_fit.py likewise).  That is the posterior of a function of the parameters.  Here the
function is a few lines of HIP that map one sample to n_out numbers:

    fn = HipFunction('''
        __device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
            out[0] = x[2] / x[1];                                            // a ratio of two parameters
            for (int k = 0; k < 64; ++k) out[1 + k] = x[0] + x[1] * p[k];    // the fitted line on 64 abscissae
        }''', n_out=65, params=t_grid)
    pd = sampler.param_est_fn(fn, n_burn=N * 500)          # pd.mean, pd.sd, pd.min, pd.max, pd.n_nan (n_out,), pd.n
    sampler.param_est_fn(fn, n_burn, values=True).values   # (rows, n_out): row r is derive(param_est(n_burn)[2][r])

x is one super-chain row (d coordinates), ll that row's stored log-likelihood, p the parameter block; out[0 .. n_out) is zero on entry, so an output
the function does not write is 0.0.  The device math functions, INFINITY, NAN and M_PI are there as for HipLikelihood's ln_like; the source is
compiled -O3 -ffp-contract=off, so a formula of + - * / gives the bits NumPy gives.

The library compiles one window-reduction kernel around the function (bpm_set_device_function / bpm_derive, bipymc_amd/csrc/derived.h); this
module validates, merges the ranks in rank order with the trace summaries' own merge (traces.merge_moments / finish: moments over the finite
values, NumPy's answer for a mean where some value is not finite, min / max over what is not NaN) and puts the values into super-chain order.
Every rank runs the same arithmetic on the same gathered parts: every rank returns the same bits.

A derived history is a history: `sampler.derived_history(fn)` writes fn of every resident row into the history of a second, ordinary handle
with dim = n_out (bpm_derive_history; the fill kernel of bipymc_amd/csrc/derive_rows.h) and returns a DerivedHistory, which carries every
statistic of _history_stats.HistoryStatistics over the derived quantities:

    with sampler.derived_history(fn) as dh:
        lo, med, hi = dh.param_est_quantiles(n_burn, q=(0.05, 0.5, 0.95))     # (3, n_out): the predictive band
        dh.convergence_diagnostics(n_burn)                                     # R-hat / ESS of every output
"""
from __future__ import division

import collections

import numpy as np

from ._history_stats import HistoryStatistics, check_n_burn, empty_window
from .comm import single_process_allgather  # noqa: F401  (for callers without a communicator)
from .traces import finish, merge_moments

WHO = "param_est_fn"
MAX_OUT = 256


class PosteriorDerived(collections.namedtuple("PosteriorDerived", ["mean", "sd", "min", "max", "n_nan", "n", "values"])):
    """mean, sd (ddof 0), min, max (n_out,): np.mean / np.std / np.nanmin / np.nanmax of each output over the window's rows; n_nan (n_out,)
    int64: how many of its values are NaN; n: rows of the window, summed over ranks; values: None, or (n, n_out) in super-chain order"""
    __slots__ = ()

    def band(self, k=1.0):
        """(mean - k sd, mean + k sd)"""
        return self.mean - k * self.sd, self.mean + k * self.sd


class HipFunction(object):
    """A function of one sample as HIP source: `source` defines

        __device__ void derive(const double* x, int d, double ll, const double* p, double* out)       // writes out[0 .. n_out)

    with 1 <= n_out <= 256; params: the float64 block `p` (as HipLikelihood's).  python_fn(X (n, d), ll (n,), params) -> (n, n_out) (optional):
    the same statement for the host -- engines that cannot compile (CPU tests) use it."""

    def __init__(self, source, n_out, params=(), python_fn=None):
        if isinstance(n_out, bool) or not isinstance(n_out, (int, np.integer)):
            raise TypeError("HipFunction: n_out must be an integer (got %r)" % (n_out,))
        if not 1 <= int(n_out) <= MAX_OUT:
            raise ValueError("HipFunction: n_out must be 1 ... %d (got %d)" % (MAX_OUT, int(n_out)))
        self.source = str(source)
        self.n_out = int(n_out)
        self.params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        self.python_fn = python_fn

    def __call__(self, X, ll):
        """the host statement on rows X (n, d) with log-likelihoods ll (n,) -> (n, n_out)"""
        if self.python_fn is None:
            raise TypeError("this HipFunction has no python_fn: it can only be evaluated on the device")
        X = np.asarray(X, dtype=np.float64)
        out = np.asarray(self.python_fn(X, np.asarray(ll, dtype=np.float64), self.params), dtype=np.float64)
        if out.shape != (len(X), self.n_out):
            raise ValueError("HipFunction: python_fn returned shape %r for %d rows and n_out = %d" % (out.shape, len(X), self.n_out))
        return out

    def check(self, arch=None):
        """Compile only (no GPU needed): raises ValueError with the compiler's log when the source does not build for `arch` (default gfx950)."""
        from ._lib import check_source
        return check_source("bpm_check_device_function", self.source.encode(), self.n_out, arch=arch)


def rank_rows(rank, n_ranks, n_chains, history_rows, n_rows, n_first, who=WHO):
    """Super-chain rows (g * n_chains + i) of a rank's window in the rank's own order: n_first rows of a partial first generation (its last
    n_first local chains), then whole generations up to the last one"""
    n_local = n_chains // n_ranks
    whole, rest = divmod(n_rows - n_first, n_local)
    if rest or not 0 <= n_first < n_local or whole + (1 if n_first else 0) > history_rows:
        raise RuntimeError("%s: rank %d reports %d rows, %d of them in a partial generation, for %d local chains and %d generations"
                           % (who, rank, n_rows, n_first, n_local, history_rows))
    g0 = history_rows - whole
    head = (g0 - 1) * n_chains + rank * n_local + (n_local - n_first) + np.arange(n_first, dtype=np.int64)
    body = (np.arange(g0, history_rows, dtype=np.int64)[:, None] * n_chains + rank * n_local + np.arange(n_local, dtype=np.int64)[None, :])
    return np.concatenate([head, body.reshape(-1)])


def gather_window(who, allgather, part, n_burn, n_chains, history_rows, k, m, values):
    """The collective frame of a statistic over the window (compute below, pointwise.compute).  part: this rank's (counts (k, m), sums (5, m),
    n_rows, n_first, values (n_rows, m) or None); allgather(obj) -> [obj of every rank] in rank order ([obj] for one process,
    single_process_allgather).  -> (counts and sums of every rank, n: the window's rows, which must be the rows >= n_burn of the super chain,
    values (n, m) in super-chain order or None)"""
    n_chains, history_rows = int(n_chains), int(history_rows)
    parts = allgather(part)
    n = sum(int(p[2]) for p in parts)
    if n == 0:
        raise empty_window(who, n_burn)
    if n != n_chains * history_rows - n_burn:
        raise RuntimeError("%s: the ranks hold %d rows of the window; rows >= %d of %d generations of %d chains are %d"
                           % (who, n, n_burn, history_rows, n_chains, n_chains * history_rows - n_burn))
    vals = None
    if values:
        vals = np.empty((n, m))
        for r, p in enumerate(parts):
            rows = rank_rows(r, len(parts), n_chains, history_rows, int(p[2]), int(p[3]), who)
            vals[rows - n_burn] = np.asarray(p[4], dtype=np.float64).reshape(len(rows), m)
    counts = [np.asarray(p[0], dtype=np.int64).reshape(k, m) for p in parts]
    sums = [np.asarray(p[1], dtype=np.float64).reshape(5, m) for p in parts]
    return counts, sums, n, vals


def compute(derive, allgather, fn, n_burn, n_chains, history_rows, values=False):
    """The collective driver.  derive(fn, n_burn, values) -> (counts (2, n_out), sums (5, n_out), n_rows, n_first, values (n_rows, n_out) or
    None) of this rank's rows (HipEngine.derive).  -> PosteriorDerived, the same bits on every rank"""
    if not isinstance(fn, HipFunction):
        raise TypeError("%s: fn must be a HipFunction (got %s)" % (WHO, type(fn).__name__))
    n_burn = check_n_burn(WHO, n_burn)
    counts, sums, n, vals = gather_window(WHO, allgather, derive(fn, n_burn, bool(values)), n_burn, n_chains, history_rows, 2, fn.n_out, values)
    n_nan = np.sum([c[1] for c in counts], axis=0)
    mn = np.min([s[3] for s in sums], axis=0)
    mx = np.max([s[4] for s in sums], axis=0)
    nf, mean, m2 = merge_moments([(c[0], s[0], s[1], s[2]) for c, s in zip(counts, sums)])
    mean, sd = finish(nf, mean, m2, n_nan, mx == np.inf, mn == -np.inf)
    some = (n - n_nan) > 0
    mn, mx = np.where(some, mn, np.nan), np.where(some, mx, np.nan)
    return PosteriorDerived(mean, sd, mn, mx, n_nan, n, vals)


class DerivedHistory(HistoryStatistics):
    """The values of a HipFunction over a sampler's history as a resident history of their own (HistoryStatistics.derived_history): with
    V = sampler.param_est_fn(fn, 0, values=True).values reshaped to (generations, n_chains, n_out), every method returns what it would return
    on a sampler whose history is V and whose log-likelihood history is the parent's.  A snapshot: it keeps describing the parent's history as
    it was when it was built.  Holds rows x (n_out rounded up to even) x 8 bytes of device memory until close(); a context manager."""

    def __init__(self, engine, n_chains, allgather):
        self._engine = engine
        self._stats_allgather = allgather
        self.n_chains = int(n_chains)
        self.n_out = self.dim = int(engine.dim)
        self.history_rows = int(engine.history_rows())

    def _stats_engine(self, who):
        if self._engine is None:
            raise RuntimeError("%s: this derived history is closed" % who)
        return self._engine

    def param_est(self, n_burn):
        """-> (mean, std, values): values = the derived quantities of the parent's super-chain rows >= n_burn, (rows, n_out)"""
        w = self._stats_engine("param_est").get_history().reshape(-1, self.n_out)[n_burn:, :]
        return np.mean(w, axis=0), np.std(w, axis=0), w

    def close(self):
        eng, self._engine = self._engine, None
        if eng is not None:
            eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
