"""Thinned histories, the host side (no GPU): the `thin` kwarg of the sampler classes is validated before any engine exists and reaches the
engine factory only when it is not the default; the rows a run reserves; the checkpoint's new fields, written and read through the oracle
engine of tests/_oracle_engine.py (which knows nothing of thinning and keeps working untouched)."""
import numpy as np
import pytest

import bipymc_amd.demc as D
from bipymc_amd import checkpoint
from bipymc_amd.demc import DeMcMpi, check_thin, stored_rows
from bipymc_amd.dream import DreamMpi
from bipymc_amd.samplers import DeMc
from bipymc_amd.utils import dblgauss_rv


@pytest.mark.parametrize("bad", [0, -1, 2.0, "3", None, True])
def test_thin_is_validated_before_any_engine_exists(monkeypatch, bad):
    made = []
    monkeypatch.setattr(D, "_engine_factory", lambda **kw: made.append(kw))
    t = dblgauss_rv.BimodeGauss_2D()
    for cls in (DeMcMpi, DreamMpi):
        with pytest.raises(ValueError, match="thin"):
            cls(t.ln_like, np.zeros(2), n_chains=8, seed=1, thin=bad)
    with pytest.raises(ValueError, match="thin"):
        DeMc(t.ln_like, n_chains=8, thin=bad)
    assert made == []
    assert check_thin(np.int64(4)) == 4 and check_thin(1) == 1


def test_the_factory_sees_no_new_keyword_at_the_default_stride(monkeypatch, oracle_engine):
    seen = []

    def factory(**kw):
        seen.append(dict(kw))
        kw.pop("thin", None)
        return oracle_engine(**kw)

    monkeypatch.setattr(D, "_engine_factory", factory)
    t = dblgauss_rv.BimodeGauss_2D()
    a = DreamMpi(t.ln_like, np.zeros(2), n_chains=8, seed=1)
    b = DreamMpi(t.ln_like, np.zeros(2), n_chains=8, seed=1, thin=1)
    c = DeMcMpi(t.ln_like, np.zeros(2), n_chains=8, seed=1, thin=5)
    assert "thin" not in seen[0] and "thin" not in seen[1] and seen[2]["thin"] == 5
    assert (a.thin, b.thin, c.thin) == (1, 1, 5)
    s = DeMc(t.ln_like, n_chains=8, seed=3)
    s.run_mcmc(8 * 4, np.zeros(2))
    assert "thin" not in seen[3] and s.thin == 1
    assert np.array_equal(s.history_generations(), np.arange(4))


def test_reservation_arithmetic():
    # stored rows of a history of L logical rows at stride k: rows 0, k, 2k, ... below L
    for L in range(1, 40):
        for k in (1, 2, 3, 7, 50):
            assert stored_rows(L, k) == len(range(0, L, k))
    assert stored_rows(100001, 10) == 10001 and stored_rows(0, 3) == 0


def test_a_run_reserves_the_rows_it_will_store(monkeypatch, oracle_engine):
    reserved = []

    class Thin3(object):
        """the oracle engine, with the two calls of a thinning engine the class asks at thin > 1"""
        def __init__(self, **kw):
            assert kw.pop("thin") == 3
            self._e = oracle_engine(**kw)

        def __getattr__(self, name):
            return getattr(self._e, name)

        def history_thin(self):
            return dict(thin=3, rows_logical=self._e.history_rows(), rows=self._e.history_rows(), last_stored=0)

        def reserve_history(self, rows):
            reserved.append(rows)

    monkeypatch.setattr(D, "_engine_factory", lambda **kw: Thin3(**kw))
    t = dblgauss_rv.BimodeGauss_2D()
    s = DeMcMpi(t.ln_like, np.zeros(2), n_chains=8, seed=1, thin=3)
    s.run_mcmc(8 * (10 + 1))                      # 10 generations from logical row 0: rows 0, 3, 6, 9
    assert reserved == [4]


def test_default_stride_reserves_a_row_per_generation(monkeypatch, oracle_engine):
    reserved = []
    real = oracle_engine

    def factory(**kw):
        e = real(**kw)
        e.reserve_history = reserved.append
        return e

    monkeypatch.setattr(D, "_engine_factory", factory)
    t = dblgauss_rv.BimodeGauss_2D()
    s = DeMcMpi(t.ln_like, np.zeros(2), n_chains=8, seed=1)
    s.run_mcmc(8 * (10 + 1))
    s.run_mcmc(8 * (5 + 1))
    assert reserved == [11, 16]


@pytest.mark.parametrize("ext", [".h5", ".npz"])
def test_checkpoint_fields_through_the_oracle_engine(tmp_path, oracle_engine, ext):
    if ext == ".h5" and checkpoint.hdf5_backend() is None:
        pytest.skip("neither h5py nor libhdf5 can be loaded on this machine")
    t = dblgauss_rv.BimodeGauss_2D()
    f = str(tmp_path / ("ck" + ext))
    s = DreamMpi(t.ln_like, np.zeros(2), n_chains=8, n_cr_gen=3, burnin_gen=10, seed=5)
    s.run_mcmc(8 * 13)
    s.save_state(f)
    hist, adapt = checkpoint.read(f, 8, 2)
    assert hist.shape == (13, 8, 2)
    assert int(adapt["thin"]) == 1 and int(adapt["rows_logical"]) == 13
    assert np.array_equal(np.asarray(adapt["state"]).reshape(8, 2), s._engine.get_state())
    assert np.array_equal(np.asarray(adapt["state"]).reshape(8, 2), hist[-1])
    assert int(adapt["t_abs"]) == 12 and int(adapt["seed"]) == 5 and len(adapt["p_cr"]) == 3      # (what was there before stays)
    # ... and loads into an engine that takes set_history(hist, X) only
    w = DreamMpi(t.ln_like, np.zeros(2), n_chains=8, n_cr_gen=3, burnin_gen=10, seed=5)
    w.load_state(f)
    assert np.array_equal(w.param_est(0)[2], s.param_est(0)[2]) and w.thin == 1
    assert np.array_equal(w.history_generations(), np.arange(13))
    # a file without the new fields (as the parent's code wrote it) reads as stride 1 with state = last row
    old = str(tmp_path / ("old" + ext))
    checkpoint.write(old, hist, {k: adapt[k] for k in ("t_abs", "seed", "p_cr", "delta_m", "n_cr_updates")})
    back, adapt_old = checkpoint.read(old, 8, 2)
    assert "thin" not in adapt_old and "state" not in adapt_old and "rows_logical" not in adapt_old
    o = DreamMpi(t.ln_like, np.zeros(2), n_chains=8, n_cr_gen=3, burnin_gen=10, seed=5)
    o.load_state(old)
    assert np.array_equal(o.param_est(0)[2], s.param_est(0)[2])
    assert np.array_equal(o._engine.get_state(), hist[-1])
    # a file of stride 3 into samplers of stride 3 k and of another stride: refused before the engine is touched when it is no multiple
    thinned = str(tmp_path / ("thin" + ext))
    checkpoint.write(thinned, hist[::3], dict(adapt, thin=3))
    calls = []
    n = DreamMpi(t.ln_like, np.zeros(2), n_chains=8, n_cr_gen=3, burnin_gen=10, seed=5)
    n._engine.set_history = lambda *a, **k: calls.append((a, k))
    n.thin = 2
    with pytest.raises(ValueError, match="multiple of 3"):
        n.load_state(thinned)
    assert calls == []
    n.thin = 6
    n._engine.thin_history = lambda m: calls.append(("thin_history", m))
    n.load_state(thinned)
    (args, kwargs), second = calls
    assert np.array_equal(args[0], hist[::3]) and np.array_equal(args[1], hist[-1])
    assert kwargs == dict(thin=3, rows_logical=13) and second == ("thin_history", 2)


def test_thin_history_of_the_classes_validates_and_follows(oracle_engine):
    t = dblgauss_rv.BimodeGauss_2D()
    s = DeMcMpi(t.ln_like, np.zeros(2), n_chains=8, seed=1)
    s.run_mcmc(8 * 7)
    with pytest.raises(ValueError, match="m must be"):
        s.thin_history(0)
    s.param_est(0)
    assert s._hist_cache is not None
    s.thin_history(1)                             # a no-op for the engine; the cached copy of the history goes all the same
    assert s.thin == 1 and s._hist_cache is None
    asked = []
    s._engine.thin_history = asked.append
    s.thin_history(4)
    assert asked == [4] and s.thin == 4
    s.thin_history(2)
    assert asked == [4, 2] and s.thin == 8
