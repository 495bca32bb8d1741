"""The statistics of a sampler's resident history, once for every sampler class: convergence diagnostics, quantiles, covariance,
histograms, per-generation traces and summaries of user-written derived quantities (bipymc_amd/diagnostics.py, quantiles.py, covariance.py,
histograms.py, traces.py, derived.py), each reduced where the history lives -- and derived_history and rank_history, which make the values
of such a function, or the pooled ranks of the window (rank_diagnostics.py), a resident history of their own, with these same methods.

The contract they share.  The window is the super-chain rows >= n_burn, param_est's selection (row g * n_chains + i = chain i at generation
g); it needs keep_history=True.  Each call is collective: every rank calls it with the same arguments, and every rank gets the same bits,
because the ranks' parts travel through one allgather and are merged in rank order.

With a thinned history (`thin=k` on the sampler, or after thin_history) the rows are the STORED rows -- every k-th generation: n_burn, `every`,
lags, tau and ESS count stored rows / stored draws, and n_burn = n_chains * r leaves out the first r stored rows (r * k generations).

A host class provides two hooks: _stats_engine(who) -> its engine (or the error of a sampler that has not run, in the name of the method
`who`), and _stats_allgather(obj) -> [obj of every rank] in rank order.
"""


def check_n_burn(who, n_burn):
    """-> int(n_burn), which must not be negative"""
    n_burn = int(n_burn)
    if n_burn < 0:
        raise ValueError("%s: n_burn must be >= 0 (got %d)" % (who, n_burn))
    return n_burn


def empty_window(who, n_burn):
    """the error of a window without rows (for the caller to raise)"""
    return ValueError("%s: the window is empty (n_burn = %d is at or beyond the last super-chain row)" % (who, int(n_burn)))


class HistoryStatistics(object):
    def convergence_diagnostics(self, n_burn=0, max_lag=None):
        """Split-chain R-hat and effective sample size per coordinate; the window starts at the first whole generation after n_burn.
        Over a thinned history n_burn, lags and tau count stored rows and ESS stored draws.  max_lag bounds the autocorrelation lags read (ess_capped says where it ended the sum).  -> diagnostics.ConvergenceDiagnostics"""
        from . import diagnostics as _diag
        eng = self._stats_engine("convergence_diagnostics")
        g0, g1 = _diag.window(n_burn, self.n_chains, eng.history_rows())
        return _diag.compute(eng.diag_split_moments, eng.diag_autocov, self._stats_allgather, g0, g1, max_lag=max_lag)

    def convergence_diagnostics_rank(self, n_burn=0, max_lag=None, prob=(0.05, 0.95)):
        """The rank-normalized split-R-hat, bulk-ESS and tail-ESS of Vehtari et al. (2021), as Stan and ArviZ report them, over
        convergence_diagnostics' window (n_burn, lags and ESS count stored rows / stored draws of a thinned history): r_hat = max(bulk, tail) sees chains that differ in scale as well as in location and is defined for
        heavy tails; ess_tail = min over the indicators x <= np.quantile(prob) says how well those quantiles are estimated.  Pooled ranks,
        normal scores and indicators are written into one scratch handle (four fills, each read by the classic pipeline), which costs the
        window's rows x (dim rounded up to even + 1) x 8 bytes plus the sort's scratch while the call runs.  Single rank only.
        -> rank_diagnostics.RankDiagnostics"""
        from . import diagnostics as _diag
        from . import rank_diagnostics as _rk
        who = "convergence_diagnostics_rank"
        _rk.check_single_rank(who, getattr(getattr(self, "comm", None), "size", 1))
        _rk.check_prob(who, prob)
        eng = self._stats_engine(who)
        g0, g1 = _diag.window(n_burn, self.n_chains, eng.history_rows())
        return _rk.compute(eng, self._stats_allgather, g0, g1, max_lag=max_lag, prob=prob, who=who)

    def rank_history(self, n_burn=0, scale="z", folded=False):
        """A ranked history is a history: the split rows of convergence_diagnostics' window (2n generations: the first and the last n of
        the window) with every value replaced by the normal score of its pooled rank within its coordinate (scale="z"), or by that average
        rank itself (scale="rank": what a rank plot bins); folded=True ranks |x - median| instead.  Kept on the device as the history of a
        second handle, so every method of this class reads it.  A snapshot; single rank only.
        -> derived.DerivedHistory (a context manager)"""
        from . import derived as _dv
        from . import diagnostics as _diag
        from . import rank_diagnostics as _rk
        who = "rank_history"
        _rk.check_single_rank(who, getattr(getattr(self, "comm", None), "size", 1))
        eng = self._stats_engine(who)
        g0, g1 = _diag.window(n_burn, self.n_chains, eng.history_rows())
        return _dv.DerivedHistory(_rk.ranked_engine(eng, g0, g1, scale=scale, folded=folded, who=who), self.n_chains, self._stats_allgather)

    def param_est_hdi(self, n_burn=0, prob=0.94):
        """The highest-density interval of every coordinate over param_est(n_burn)[2]: the shortest interval that holds the share `prob` of
        the draws -- with the S values sorted and m = min(floor(prob * S), S - 1), the first i of the smallest s[i + m] - s[i] gives
        (s[i], s[i + m]) (summary.py has the definition with its NaN and inf rules).  prob: one probability or up to 8.  One sort of every
        column on the device and one scan per probability.  Single rank only.  -> summary.PosteriorHDI(lo, hi, prob, n_nan, n)"""
        from . import rank_diagnostics as _rk
        from . import summary as _sm
        who = "param_est_hdi"
        _rk.check_single_rank(who, getattr(getattr(self, "comm", None), "size", 1))
        _sm.check_hdi_prob(who, prob)
        return _sm.compute_hdi(self._stats_engine(who), n_burn, prob, self.n_chains, who=who)

    def posterior_summary(self, n_burn=0, hdi_prob=0.94, prob=(0.05, 0.95), max_lag=None):
        """The table a Bayesian report prints, per coordinate: mean, sd, the highest-density interval of hdi_prob, median and
        np.quantile(prob), the Monte Carlo standard errors of mean and sd, ess_mean, ess_sd, ess_bulk, ess_tail, the rank-normalized and the
        classic R-hat -- all over the split rows of convergence_diagnostics' window, the same draws in every column (n_burn, lags and ESS
        count stored rows / stored draws of a thinned history).  str() of the result is the table.  Costs what convergence_diagnostics_rank
        costs plus one sort of the raw columns and a fifth fill of its one scratch handle.  Single rank only.
        -> summary.PosteriorSummary"""
        from . import diagnostics as _diag
        from . import rank_diagnostics as _rk
        from . import summary as _sm
        who = "posterior_summary"
        _rk.check_single_rank(who, getattr(getattr(self, "comm", None), "size", 1))
        _rk.check_prob(who, prob)
        _sm.check_hdi_prob(who, hdi_prob)
        eng = self._stats_engine(who)
        g0, g1 = _diag.window(check_n_burn(who, n_burn), self.n_chains, eng.history_rows())
        return _sm.compute(eng, self._stats_allgather, g0, g1, hdi_prob=hdi_prob, prob=prob, max_lag=max_lag, who=who)

    def param_est_quantiles(self, n_burn=0, q=(0.05, 0.5, 0.95)):
        """np.quantile(param_est(n_burn)[2], q, axis=0), exactly (an MSD radix select).  -> (len(q), dim), or (dim,) for a scalar q"""
        from . import quantiles as _qs
        eng = self._stats_engine("param_est_quantiles")
        return _qs.compute(eng.quantile_begin, eng.quantile_histogram, self._stats_allgather, n_burn, q, dim=eng.dim)

    def param_est_cov(self, n_burn=0):
        """Posterior mean, covariance (ddof = 1) and, through .corr(), correlation: what np.cov(param_est(n_burn)[2], rowvar=False)
        computes (an FP64 matrix-core SYRK centred on the global mean).  -> covariance.PosteriorCovariance(mean, cov, n)"""
        from . import covariance as _cov
        eng = self._stats_engine("param_est_cov")
        return _cov.compute(eng.reduce_moments, eng.reduce_cov, self._stats_allgather, n_burn, eng.dim)

    def param_est_hist(self, n_burn=0, bins=20, range=None, dims=None, pairs=None, bins2d=None):
        """The counts of a corner plot: per coordinate of `dims` (None: all) exactly np.histogram(param_est(n_burn)[2][:, k], bins,
        range)[0], per pair of `pairs` (None: none; "all": every a < b of dims; or (a, b) tuples) exactly np.histogram2d(..., bins2d,
        range=[ra, rb])[0].  range: None for each coordinate's (min, max), (lo, hi) for all, or one (lo, hi) per coordinate.
        -> histograms.PosteriorHistograms(dims, edges, counts, pairs, edges2d, counts2d, n) with .density()"""
        from . import histograms as _hs
        eng = self._stats_engine("param_est_hist")
        return _hs.compute(eng.hist_range, eng.hist_marginals, eng.hist_pairs, self._stats_allgather, n_burn, eng.dim, bins=bins,
                           range=range, dims=dims, pairs=pairs, bins2d=bins2d)

    def param_est_trace(self, n_burn=0, every=1, chains=None):
        """What a trace plot shows, per bin of `every` generations from the first whole generation at or after n_burn: mean, sd (np.mean /
        np.std of the bin's rows), min, max and NaN count per coordinate, mean / min / max of the log-likelihood, the best sample of the
        window, and the global chains `chains` (None: none) at the first generation of every bin -- the picture the reference draws from
        param_est(n_burn=0)'s copy of the history.  -> traces.PosteriorTrace with .band(k)"""
        from . import traces as _tr
        eng = self._stats_engine("param_est_trace")
        return _tr.compute(eng.trace_bins, eng.trace_chains, self._stats_allgather, n_burn, self.n_chains, eng.history_rows(), eng.dim,
                           every=every, chains=chains)

    def param_est_fn(self, fn, n_burn=0, values=False):
        """The posterior of a function of the parameters: `fn` (a derived.HipFunction: a few lines of HIP mapping one sample and its
        log-likelihood to n_out numbers) over param_est(n_burn)[2]'s rows -- np.mean, np.std, np.nanmin, np.nanmax and the NaN count of every
        output, and with values=True the (rows, n_out) matrix itself in super-chain order; what the reference's fitting scripts compute on the
        host from param_est's copy of the history.  -> derived.PosteriorDerived(mean, sd, min, max, n_nan, n, values) with .band(k)"""
        from . import derived as _dv
        eng = self._stats_engine("param_est_fn")
        return _dv.compute(eng.derive, self._stats_allgather, fn, n_burn, self.n_chains, eng.history_rows(), values=values)

    def param_est_waic(self, pw, n_burn=0, values=False):
        """WAIC and the pointwise expected log predictive density: `pw` (a pointwise.HipPointwise: the log density of ONE datum as a few
        lines of HIP, with the data) over param_est(n_burn)[2]'s rows -- per datum log mean exp, variance and mean of its log densities
        over the draws, the totals elpd_waic, p_waic, lppd, se and waic, the counts of what is not finite, and with values=True the
        (rows, n_data) matrix itself in super-chain order.  Independent of how the sampler's likelihood was given.  Two results over the
        same data compare with pointwise.compare_waic.  -> pointwise.PosteriorWaic; str() of it is a short table"""
        from . import pointwise as _pw
        eng = self._stats_engine("param_est_waic")
        return _pw.compute(eng.pointwise, self._stats_allgather, pw, n_burn, self.n_chains, eng.history_rows(), values=values)

    def param_est_loo(self, pw, n_burn=0, r_eff=1.0, tails=False):
        """PSIS-LOO, the leave-one-out expected log predictive density with its Pareto-k diagnostic per datum: `pw` (the HipPointwise of
        param_est_waic) over param_est(n_burn)[2]'s rows -- per datum elpd_loo_i, pareto_k (above 0.7: the estimate for this datum cannot be
        trusted; it is an outlier or has leverage), lppd_i (param_est_waic's bits), p_loo_i and tail_len, the totals elpd_loo, p_loo, se,
        looic and n_bad_k; with tails=True each datum's kept values too.  r_eff: the relative efficiency of the draws, a scalar or one per
        datum, > 0; it only sets the tail length M = ceil(min(S / 5, 3 sqrt(S / r_eff))).  1.0 is what ArviZ assumes when it is not told; a
        DREAM or DE-MC population's draws are autocorrelated, and convergence_diagnostics(...).ess of derived_history(exp(l)) divided by
        the draws n is a way to obtain it.  Each datum's tail is selected exactly on the device, in scratch of at most BPM_LOO_SCRATCH_MB
        (by default a quarter of the free memory); kept sets that cannot fit are refused with advice.  Two results over the same data
        compare with pointwise.compare_loo.  Single rank only.  -> pointwise.PosteriorLoo; str() of it is a short table"""
        from . import pointwise as _pw
        from . import rank_diagnostics as _rk
        who = "param_est_loo"
        _rk.check_single_rank(who, getattr(getattr(self, "comm", None), "size", 1))
        eng = self._stats_engine(who)
        return _pw.compute_loo(eng, self._stats_allgather, pw, n_burn, self.n_chains, r_eff=r_eff, tails=tails)

    def derived_history(self, fn):
        """A derived history is a history: `fn` (a derived.HipFunction) over every resident row, kept on the device as the history of a
        second handle with dim = fn.n_out and this sampler's log-likelihoods -- so every method of this class answers about the derived
        quantities: param_est_quantiles for the 5 / 50 / 95 % predictive band, convergence_diagnostics for R-hat and ESS of the quantity one
        reports, param_est_hist, param_est_cov, param_est_trace and param_est_fn (a function of derived quantities).  A snapshot of the
        history as it is now; costs rows x (n_out rounded up to even) x 8 bytes of device memory until closed.  Single rank only.
        -> derived.DerivedHistory (a context manager: `with sampler.derived_history(fn) as dh: ...`)"""
        from . import derived as _dv
        who = "derived_history"
        if not isinstance(fn, _dv.HipFunction):
            raise TypeError("%s: fn must be a HipFunction (got %s)" % (who, type(fn).__name__))
        n_ranks = int(getattr(getattr(self, "comm", None), "size", 1))
        if n_ranks != 1:
            raise NotImplementedError("%s: a derived history is built on a single rank only (this communicator has %d ranks)" % (who, n_ranks))
        eng = self._stats_engine(who)
        return _dv.DerivedHistory(eng.derive_history(fn), self.n_chains, self._stats_allgather)
