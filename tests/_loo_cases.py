"""What the tests of tests/test_gpu_loo.py share: the device call, the checks of its three stages against the matrix L = l_is the device itself
returns (param_est_waic(values=True)), and histories whose rows arrive in a chosen order.

THE CHECKS and where their bounds come from (nothing was tuned on the output of the code under test):
  tails        bit for bit np.sort(L[:, i])[:K_i] (of the finite values, where a datum has others), K_i from the restatement's own tail-length function (_psis_restatement.kept).
  body         body_n = S - tail_len exactly; body_m + log(body_s) against mpmath's logsumexp(-l) over the rows with l >= the cutoff, within
               _waic_cases.lppd_bound(rows per part, parts, 1, value) of the second pass's own layout -- the derivation there covers an online
               (m, s) over a part's rows and the fold of the parts, which is what the pass is.
  fit, finish  pareto_k, sigma, elpd_loo_i against _psis_restatement.fit_from_tail_exact (mpmath, 200 bits) on stage C's OWN inputs -- the device's
               sorted tail and the device's body (count, m, s) -- within the gate of profiles/psis_bound.txt: per quantity 4 x the largest error
               of the float64 NumPy restatement on the host's cases (tests/test_psis_host.py says why 4), read from that file, with no other
               term; the restatement's own error on the test's columns must lie within that gate too.  tail_len for equality.
               (With the gate measured on synthetic tails alone, 3.399e-14 for k, the window of 21 rows -- a tail of 5 -- missed it: the
               restatement's own k was off by 3.486e-14 there, the device's, and psis.h's on the host, by 4.197e-14.  The host's cases now hold
               those columns, so the recorded gate is measured where the fit is worst conditioned: 1.394e-13.)
  totals       elpd_loo, p_loo, lppd, se, looic, n_bad_k: the NumPy expressions of the per-datum arrays, bit for bit; lppd_i and the
               counters: param_est_waic's bits."""
import numpy as np

import _psis_restatement as PR
import _waic_cases as WC

N, G = 16, 130            # 2080 rows


def waic(eng, pw, n_burn=0, values=True):
    from bipymc_amd import pointwise as PW
    return PW.compute(eng.pointwise, PW.single_process_allgather, pw, n_burn, eng.n_chains, eng.history_rows(), values=values)


def loo(eng, pw, n_burn=0, r_eff=1.0, tails=True):
    from bipymc_amd import pointwise as PW
    return PW.compute_loo(eng, PW.single_process_allgather, pw, n_burn, eng.n_chains, r_eff=r_eff, tails=tails)


def installed(X):
    from _history_cases import _engine
    e = _engine(X.shape[1], X.shape[2])
    e.set_history(X, X[-1])
    assert np.array_equal(e.get_history(), X)
    return e


def r_eff_of(r_eff, n_data):
    return np.full(n_data, float(r_eff)) if np.ndim(r_eff) == 0 else np.asarray(r_eff, dtype=np.float64)


def check_tails(res, L, r_eff=1.0, what=""):
    S, nd = L.shape
    r = r_eff_of(r_eff, nd)
    assert res.n == S and len(res.tails) == nd, what
    for i in range(nd):
        K = PR.kept(S, r[i])
        col = L[:, i]
        WC.bits_equal(res.tails[i], np.sort(col[np.isfinite(col)])[:K], (what, "tail of datum", i, "K", K))      # (the kept set is of the finite values)
    assert res.stats["k_max"] == max(PR.kept(S, x) for x in r), what


def check_body(res, L, r_eff=1.0, what=""):
    import mpmath as mp
    S, nd = L.shape
    r = r_eff_of(r_eff, nd)
    worst = 0.0
    for i in range(nd):
        col = L[:, i]
        if not np.isfinite(col).all():
            continue
        tail, body = PR.split(col, r[i])
        assert res.stats["body_n"][i] == len(body) == S - res.tail_len[i], (what, i)
        exact = PR.body_lse_exact(body)
        with mp.workprec(200):
            got = mp.mpf(float(res.stats["body_m"][i])) + mp.log(mp.mpf(float(res.stats["body_s"][i])))
            err = float(abs(got - exact))
        bound = WC.lppd_bound(res.stats["body_rows_per_part"], res.stats["body_parts"], 1, float(exact))
        worst = max(worst, err / bound)
        assert err <= bound, (what, i, "body log-sum-exp", err, bound)
    print("%s: body log-sum-exp, largest error / bound %.3g (parts %d of %d rows)" % (what, worst, res.stats["body_parts"], res.stats["body_rows_per_part"]))


def check_fit(res, L, r_eff=1.0, what=""):
    """stage C on ITS inputs: the device's sorted tails (check_tails has compared them with L bit for bit) and the device's body (count, m, s)
    go into the mpmath reference and into the NumPy restatement, as the host test hands psis.h its inputs; the second pass's own rounding is
    check_body's business and is not charged here"""
    import mpmath as mp
    S, nd = L.shape
    bound = PR.recorded_bound()
    ref_err, dev_err, cols = [], [], []
    for i in range(nd):
        if not np.isfinite(L[:, i]).all():
            assert np.isnan(res.pareto_k[i]) and np.isnan(res.elpd_loo_i[i]) and np.isnan(res.p_loo_i[i]) and res.tail_len[i] == 0, (what, i)
            continue
        n_b, m_b, s_b = int(res.stats["body_n"][i]), float(res.stats["body_m"][i]), float(res.stats["body_s"][i])
        with mp.workprec(200):
            lse = mp.mpf(m_b) + mp.log(mp.mpf(s_b))
        ex = dict(PR.fit_from_tail_exact(res.tails[i], n_b, lse), smoothed=[])
        mine = dict(PR.fit_from_tail(res.tails[i], n_b, m_b + np.log(s_b)), smoothed=[])
        got = dict(k=res.pareto_k[i], sigma=res.stats["sigma"][i], tail_len=int(res.tail_len[i]), smoothed=[], elpd=res.elpd_loo_i[i])
        ref_err.append(PR.errors(mine, ex))
        dev_err.append(PR.errors(got, ex))
        cols.append(i)
    if not cols:
        return
    ref_err, dev_err = np.array(ref_err), np.array(dev_err)
    for q in (0, 1, 3):
        name = PR.QUANTITIES[q]
        gate = bound[name][1]
        print("%s: %-34s NumPy restatement %.3e, device %.3e, gate %.3e" % (what, name, ref_err[:, q].max(), dev_err[:, q].max(), gate))
        # the gate was measured on the host's cases: it says something about these columns only where the float64 restatement itself meets it here
        assert ref_err[:, q].max() <= gate, (what, name, "the restatement's own error on these columns is beyond the recorded gate", ref_err[:, q].max(), gate)
        assert dev_err[:, q].max() <= gate, (what, name, cols[int(np.argmax(dev_err[:, q]))], dev_err[:, q].max(), gate)


def check_totals(res, w, what=""):
    """w: param_est_waic's result over the same window"""
    for f in ("lppd_i", "n_nan", "n_neg_inf", "n_pos_inf"):
        WC.bits_equal(np.asarray(getattr(res, f), dtype=np.float64), np.asarray(getattr(w, f), dtype=np.float64), (what, f))
    assert res.tail_len.dtype == np.int64 and res.n == w.n
    nd = len(res.lppd_i)
    with np.errstate(all="ignore"):
        WC.bits_equal(res.p_loo_i, res.lppd_i - res.elpd_loo_i, (what, "p_loo_i"))
        WC.bits_equal([res.elpd_loo, res.p_loo, res.lppd], [np.sum(res.elpd_loo_i), np.sum(res.p_loo_i), np.sum(res.lppd_i)], (what, "totals"))
        WC.bits_equal([res.se, res.looic], [np.sqrt(nd * np.var(res.elpd_loo_i)), -2.0 * np.sum(res.elpd_loo_i)], (what, "se, looic"))
        assert res.n_bad_k == int(np.count_nonzero(res.pareto_k > 0.7)), what


def same_loo(a, b, what="", skip=()):
    keep = np.ones(len(a.lppd_i), dtype=bool)
    keep[list(skip)] = False
    for f in ("elpd_loo_i", "pareto_k", "lppd_i", "p_loo_i", "tail_len", "n_nan", "n_neg_inf", "n_pos_inf"):
        WC.bits_equal(np.asarray(getattr(a, f), dtype=np.float64)[keep], np.asarray(getattr(b, f), dtype=np.float64)[keep], (what, f))
    for f in ("body_n", "body_m", "body_s", "sigma"):
        WC.bits_equal(np.asarray(a.stats[f], dtype=np.float64)[keep], np.asarray(b.stats[f], dtype=np.float64)[keep], (what, f))
    if a.tails is not None and b.tails is not None:
        for i in np.flatnonzero(keep):
            WC.bits_equal(a.tails[i], b.tails[i], (what, "tails", i))
    assert a.n == b.n, what
    if not len(skip):
        for f in ("elpd_loo", "p_loo", "lppd", "se", "looic"):
            WC.bits_equal([getattr(a, f)], [getattr(b, f)], (what, f))
        assert a.n_bad_k == b.n_bad_k, what


# ---- histories whose last coordinate decides the order of every datum's values ---------------------------------------------------------
ORDER_PARAMS = [0.75, 1.0e5, 0.001]      # source 1: l = -0.375 (y - x0)^2 + 1e5 x[d - 1] - 0.001 i; x[d - 1] on a grid of step ~1e-3: steps of 100 in l


def ordered_history(order, ties=None):
    """(G, N, 3) of make_history with x[2] = a grid over [-1, 1] in row order `order` ("descending", "ascending" or "shuffled"); ties = (first
    rank, count): the rows holding the `count` values of x[2] from rank `first rank` (0 = smallest) on are made copies of the first of them"""
    X = WC.make_history(G, N, 3, seed=3)
    flat = X.reshape(-1, 3)
    grid = np.linspace(-1.0, 1.0, len(flat))
    if order == "descending":
        grid = grid[::-1].copy()
    elif order == "shuffled":
        grid = np.random.RandomState(11).permutation(grid)
    flat[:, 2] = grid
    if ties is not None:
        rows = np.argsort(flat[:, 2])[ties[0]:ties[0] + ties[1]]
        flat[rows] = flat[rows[0]]
    return X
