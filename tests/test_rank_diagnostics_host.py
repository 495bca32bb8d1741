"""Rank-normalized diagnostics, host side (no GPU): bipymc_amd/rank_diagnostics.py's driver over a NumPy / SciPy stand-in for
bpm_rank_history (tests/_rank_restatement.py: rankdata, ndtri, np.median, np.quantile), in the manner of DiagOracleEngine in
tests/test_diagnostics_host.py.  The stand-in serves the order statistics from a sort of its own, so the driver's median and np.quantile
interpolation are under test as well; its transformed histories are the restatement's, so every field must equal
test_diagnostics_host.reference of the transformed array to rounding (1e-12: the finishing layer against the FFT restatement, as in
test_diagnostics_host).  Also: the window (odd, n_burn that is no multiple of n_chains), degenerate coordinates, prob validation, the refusal
on two ranks before the engine is touched, and the scratch handle's life."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _rank_restatement as RR  # noqa: E402
from bipymc_amd import rank_diagnostics as RK  # noqa: E402
from bipymc_amd._history_stats import HistoryStatistics  # noqa: E402
from test_diagnostics_host import BlockParts, _ar1  # noqa: E402


class FakeRanked(object):
    """the scratch handle: the two diagnostic reductions over whatever history the last fill left"""

    def __init__(self, log):
        self.closed, self.log, self.H, self.fail_diag = 0, log, None, False

    def diag_split_moments(self, a, b):
        if self.fail_diag:
            raise RuntimeError("bpm_diag_split_moments: failed on purpose")
        self._dg = BlockParts(self.H)
        return self._dg.split(a, b)

    def diag_autocov(self, t0, nl):
        return self._dg.autocov(t0, nl)

    dim = property(lambda self: self.H.shape[2])

    def history_rows(self):
        return self.H.shape[0]

    def get_history(self):
        return self.H.copy()

    def close(self):
        self.closed += 1


class FakeRankEngine(object):
    """one rank's engine over the history X (G, N, d): rank_history as HipEngine.rank_history, stated with rankdata and ndtri"""

    def __init__(self, X, fail_at=None, fail_diag_at=None):
        self.X = np.asarray(X, dtype=np.float64)
        self.n_chains, self.dim = self.X.shape[1], self.X.shape[2]
        self.calls, self.made = [], []
        self.fail_at, self.fail_diag_at = fail_at, fail_diag_at

    def history_rows(self):
        return self.X.shape[0]

    def rank_history(self, g_lo, g_hi, kind, arg=None, positions=(), dst=None):
        self.calls.append((g_lo, g_hi, kind, None if arg is None else np.array(arg), tuple(int(p) for p in positions), dst))
        if (g_hi - g_lo) // 2 < 4:
            raise RuntimeError("bpm_rank_history: at least 4 are needed")
        if self.fail_at == len(self.calls):
            raise RuntimeError("bpm_rank_history: failed on purpose")
        W = RR.split_rows(self.X[:g_hi], g_lo)
        with np.errstate(invalid="ignore"):
            V = np.abs(W - np.asarray(arg)) if kind in (RK.KIND_Z_FOLDED, RK.KIND_RANK_FOLDED) else W
            if kind == RK.KIND_INDICATOR:
                out = (W <= np.asarray(arg)).astype(np.float64)
            else:
                r = RR.ranks(V)
                out = r if kind in (RK.KIND_RANK, RK.KIND_RANK_FOLDED) else RR.z_of(r)
        srt = np.sort(V.reshape(-1, self.dim), axis=0)                    # (NaN last, as the device's keys)
        if dst is None:
            dst = FakeRanked(self.calls)
            self.made.append(dst)
        dst.H = out
        dst.fail_diag = self.fail_diag_at == len(self.calls)
        return dst, srt[list(positions)] if len(positions) else np.empty((0, self.dim))


class Comm(object):
    def __init__(self, size):
        self.size, self.rank = size, 0


class Sampler(HistoryStatistics):
    def __init__(self, engine, comm=None):
        self._engine, self.n_chains = engine, engine.n_chains if engine is not None else 8
        self.asked = []
        if comm is not None:
            self.comm = comm

    def _stats_engine(self, who):
        self.asked.append(who)
        if self._engine is None:
            raise RuntimeError("%s: run_mcmc first" % who)
        return self._engine

    def _stats_allgather(self, obj):
        return [obj]


def _check(got, X, g0=0, prob=RR.PROB, max_lag=None):
    return RR.check_diagnostics(got, X, g0, prob, max_lag, r_hat_rtol=1e-12, ess_rtol=1e-12)


def _history(G=81, N=8, seed=3):
    X = _ar1(G, N, [0.0, 0.5, 0.9, 0.3, -0.2], seed=seed)
    X[:, :4, 3] *= 3.0                                   # half the chains wider on one coordinate: only the folded R-hat sees it
    return X


def test_every_field_equals_the_reference_of_its_transformed_array():
    X = _history()
    e = FakeRankEngine(X)
    got = Sampler(e).convergence_diagnostics_rank()
    _check(got, X)
    assert got._fields == ("r_hat", "r_hat_bulk", "r_hat_tail", "ess_bulk", "ess_tail", "ess_lower", "ess_upper", "median", "quantiles",
                           "ess_capped", "n_half_chains", "n_draws", "window")
    assert np.array_equal(got.r_hat, np.maximum(got.r_hat_bulk, got.r_hat_tail))
    assert np.array_equal(got.ess_tail, np.minimum(got.ess_lower, got.ess_upper))
    assert got.r_hat_tail[3] > 1.05 > got.r_hat_bulk[3] and not got.ess_capped.any()
    # four fills into ONE scratch handle, closed once
    assert [c[2] for c in e.calls] == [RK.KIND_Z, RK.KIND_Z_FOLDED, RK.KIND_INDICATOR, RK.KIND_INDICATOR]
    assert len(e.made) == 1 and e.made[0].closed == 1 and e.calls[0][5] is None and all(c[5] is e.made[0] for c in e.calls[1:])
    assert np.array_equal(e.calls[1][3], got.median) and np.array_equal(e.calls[2][3], got.quantiles[0])
    assert np.array_equal(e.calls[3][3], got.quantiles[1])


def test_an_odd_window_drops_its_middle_row_and_n_burn_rounds_up_to_a_generation():
    X = _history(G=80)
    e = FakeRankEngine(X)
    got = Sampler(e).convergence_diagnostics_rank(n_burn=8 * 2 + 3)       # -> g0 = 3: 77 rows, n = 38, row 3 + 38 dropped
    assert got.window == (3, 80) and got.n_draws == 38 and e.calls[0][:2] == (3, 80)
    t = _check(got, X, g0=3)
    assert np.array_equal(t["split"], np.concatenate([X[3:41], X[42:80]]))
    dropped = X[41].copy()
    X2 = X.copy()
    X2[41] = 1e6                                                           # the dropped row does not matter
    got2 = Sampler(FakeRankEngine(X2)).convergence_diagnostics_rank(n_burn=19)
    assert np.array_equal(got2.ess_bulk, got.ess_bulk) and np.array_equal(got2.quantiles, got.quantiles) and np.array_equal(X[41], dropped)
    assert Sampler(FakeRankEngine(X)).convergence_diagnostics_rank(n_burn=16).window == (2, 80)


def test_max_lag_and_other_probabilities():
    X = _ar1(201, 8, [0.95, 0.0], seed=7)
    got = Sampler(FakeRankEngine(X)).convergence_diagnostics_rank(max_lag=6, prob=(0.1, 0.75))
    _check(got, X, prob=(0.1, 0.75), max_lag=6)
    assert got.ess_capped[0]


def test_constant_nan_and_infinite_coordinates():
    X = _ar1(61, 8, [0.5, 0.5, 0.5, 0.5, 0.5], seed=2)
    X[:, :, 1] = 2.5                                     # constant
    X[7, 3, 2] = np.nan                                  # one NaN in the window
    X[5, 1, 3], X[50, 2, 3], X[51, 2, 3] = np.inf, -np.inf, -np.inf        # ordinary values for the ranks
    X[30, 0, 4] = np.nan                                 # the dropped middle row: not in the window
    got = Sampler(FakeRankEngine(X)).convergence_diagnostics_rank()
    _check(got, X)
    for name in RR.FIELDS:
        f = getattr(got, name)
        assert np.isnan(f[[1, 2]]).all() and np.isfinite(f[[0, 3, 4]]).all(), (name, f)
    assert got.median[1] == 2.5 and np.isnan(got.median[2]) and np.isnan(got.quantiles[:, 2]).all() and np.isfinite(got.median[[0, 3, 4]]).all()


@pytest.mark.parametrize("prob", [(0.95, 0.05), (0.0, 0.9), (0.1, 1.0), (0.5, 0.5), 0.05, (0.1, 0.5, 0.9), ("a", "b"), (np.nan, 0.9)])
def test_prob_is_validated_before_the_engine_is_touched(prob):
    s = Sampler(FakeRankEngine(_history()))
    with pytest.raises(ValueError, match="convergence_diagnostics_rank: prob must"):
        s.convergence_diagnostics_rank(prob=prob)
    assert s.asked == [] and s._engine.calls == []


def test_two_ranks_are_refused_before_any_engine_call():
    e = FakeRankEngine(_history())
    s = Sampler(e, comm=Comm(2))
    with pytest.raises(NotImplementedError, match=r"convergence_diagnostics_rank: pooled ranks are built on a single rank only \(this "
                                                  r"communicator has 2 ranks\)"):
        s.convergence_diagnostics_rank()
    with pytest.raises(NotImplementedError, match=r"rank_history: pooled ranks are built on a single rank only \(this communicator has 2 ranks\)"):
        s.rank_history()
    assert s.asked == [] and e.calls == []
    one = Sampler(e, comm=Comm(1))
    assert one.convergence_diagnostics_rank().n_half_chains == 16 and one.asked == ["convergence_diagnostics_rank"]


@pytest.mark.parametrize("fail_at", [1, 2, 3, 4])
def test_the_scratch_handle_is_closed_when_a_fill_raises(fail_at):
    e = FakeRankEngine(_history(), fail_at=fail_at)
    with pytest.raises(RuntimeError, match="bpm_rank_history: failed on purpose"):
        Sampler(e).convergence_diagnostics_rank()
    assert len(e.calls) == fail_at and len(e.made) == (0 if fail_at == 1 else 1) and all(h.closed == 1 for h in e.made)


@pytest.mark.parametrize("fail_diag_at", [1, 2, 3, 4])
def test_the_scratch_handle_is_closed_when_a_diagnostics_pass_raises(fail_diag_at):
    e = FakeRankEngine(_history(), fail_diag_at=fail_diag_at)
    with pytest.raises(RuntimeError, match="bpm_diag_split_moments: failed on purpose"):
        Sampler(e).convergence_diagnostics_rank()
    assert len(e.calls) == fail_diag_at and len(e.made) == 1 and e.made[0].closed == 1


def test_too_short_a_window_is_the_fills_error_and_a_sampler_that_has_not_run_its_own():
    with pytest.raises(RuntimeError, match="at least 4"):
        Sampler(FakeRankEngine(_ar1(7, 8, [0.5], seed=1))).convergence_diagnostics_rank()
    with pytest.raises(RuntimeError, match="convergence_diagnostics_rank: run_mcmc first"):
        Sampler(None).convergence_diagnostics_rank()


@pytest.mark.parametrize("scale,folded,name", [("z", False, "bulk"), ("z", True, "folded"), ("rank", False, "rank"), ("rank", True, "rank_folded")])
def test_rank_history_is_a_history_with_every_statistic(scale, folded, name):
    from bipymc_amd import DerivedHistory
    X = _history(G=80)
    e = FakeRankEngine(X)
    t = RR.restate(X, g0=3)
    with Sampler(e).rank_history(n_burn=17, scale=scale, folded=folded) as rh:
        assert isinstance(rh, DerivedHistory) and (rh.history_rows, rh.n_chains, rh.dim) == (76, 8, 5)
        assert np.array_equal(rh.param_est(0)[2], t[name].reshape(-1, 5))
        d = rh.convergence_diagnostics(0)
        assert d.n_draws == 38 and np.isfinite(d.r_hat).all()
    assert len(e.made) == 1 and e.made[0].closed == 1
    with pytest.raises(ValueError, match="rank_history: scale must be 'z' or 'rank'"):
        Sampler(e).rank_history(scale="u")
    if folded:                                            # the first fill's handle is closed when the second raises
        bad = FakeRankEngine(X, fail_at=2)
        with pytest.raises(RuntimeError, match="failed on purpose"):
            Sampler(bad).rank_history(scale=scale, folded=True)
        assert len(bad.made) == 1 and bad.made[0].closed == 1


def test_the_abi_declares_the_entry_point():
    from bipymc_amd import _lib as L
    lib = L.load()
    assert "bpm_rank_history" in L.SIGNATURES and "csrc/ranks.h" in L._ID_SRCS
    assert lib.bpm_rank_history(None, None, 0, 0, 0, None, 0, None, None) != 0 and b"bpm_rank_history: null handle" in lib.bpm_last_error()
