"""One rank of a world of processes sharing one GPU for tests/test_gpu_histograms.py: DreamMpi over the push exchange, then the collective
param_est_hist (and, on rank 0 of a one-rank world, the history np.histogram / np.histogram2d are taken over).
usage: _histogram_worker.py <dir> <rank> <world>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

N_BURN = 64 * 10 + 3
KW = dict(bins=20, pairs=[(0, 1), (9, 2), (4, 5)], bins2d=12)


def run(comm):
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.5, dim=10)
    s = DreamMpi(t.ln_like, np.zeros(10), n_chains=64, mpi_comm=comm, n_cr_gen=3, burnin_gen=10, seed=77,
                 exchange="push" if comm is not None else "auto")
    s.run_mcmc(64 * 60)
    ph = s.param_est_hist(N_BURN, **KW)
    out = {"edges": ph.edges, "counts": ph.counts, "edges2d": ph.edges2d, "counts2d": ph.counts2d, "n": np.int64(ph.n)}
    if comm is None:
        out["chain_slice"] = s.param_est(N_BURN)[2]
    return out


def main():
    d_, rank, world = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    comm = None
    if world > 1:
        from _file_comm import FileComm
        comm = FileComm(d_, rank, world)
    out = run(comm)
    np.savez(os.path.join(d_, "hs_w%d_rank%d.npz" % (world, rank)), **out)


if __name__ == "__main__":
    main()
