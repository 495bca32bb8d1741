"""One rank of a world of processes sharing one GPU for tests/test_gpu_{diagnostics,quantiles,covariance,histograms}.py: DreamMpi over the
push exchange, then one collective statistic of the history (and, on rank 0 of a one-rank world, the history NumPy's answer is taken over).
usage: _stats_worker.py <stat> <dir> <rank> <world>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

N_BURN = 64 * 10 + 3
Q = [0.0, 0.05, 0.5, 0.95, 1.0]
KW = dict(bins=20, pairs=[(0, 1), (9, 2), (4, 5)], bins2d=12)


def _diag(s):
    res = s.convergence_diagnostics(n_burn=N_BURN)
    return {f: np.asarray(getattr(res, f)) for f in res._fields}


def _quantiles(s):
    return {"q": s.param_est_quantiles(N_BURN, Q)}


def _cov(s):
    pc = s.param_est_cov(N_BURN)
    return {"cov": pc.cov, "mean": pc.mean, "n": np.int64(pc.n)}


def _hist(s):
    ph = s.param_est_hist(N_BURN, **KW)
    return {"edges": ph.edges, "counts": ph.counts, "edges2d": ph.edges2d, "counts2d": ph.counts2d, "n": np.int64(ph.n)}


# stat -> (the call and its output dictionary, prefix of the .npz name, whether a one-rank world also saves param_est's rows)
STATS = {"diag": (_diag, "diag", False), "quantiles": (_quantiles, "qs", True), "cov": (_cov, "cov", True), "hist": (_hist, "hs", True)}


def run(stat, comm):
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    call, _, with_rows = STATS[stat]
    t = d100_gauss.Gauss_100D(rho=0.5, dim=10)
    s = DreamMpi(t.ln_like, np.zeros(10), n_chains=64, mpi_comm=comm, n_cr_gen=3, burnin_gen=10, seed=77,
                 exchange="push" if comm is not None else "auto")
    s.run_mcmc(64 * 60)
    out = call(s)
    if with_rows and comm is None:
        out["chain_slice"] = s.param_est(N_BURN)[2]
    return out


def main():
    stat, d_, rank, world = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    comm = None
    if world > 1:
        from _file_comm import FileComm
        comm = FileComm(d_, rank, world)
    out = run(stat, comm)
    np.savez(os.path.join(d_, "%s_w%d_rank%d.npz" % (STATS[stat][1], world, rank)), **out)


if __name__ == "__main__":
    main()
