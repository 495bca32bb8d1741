"""One rank of a world of processes sharing one GPU for tests/test_gpu_covariance.py: DreamMpi over the push exchange, then the collective
param_est_cov (and, on rank 0 of a one-rank world, the history np.cov is taken over).
usage: _covariance_worker.py <dir> <rank> <world>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

N_BURN = 64 * 10 + 3


def run(comm):
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.5, dim=10)
    s = DreamMpi(t.ln_like, np.zeros(10), n_chains=64, mpi_comm=comm, n_cr_gen=3, burnin_gen=10, seed=77,
                 exchange="push" if comm is not None else "auto")
    s.run_mcmc(64 * 60)
    pc = s.param_est_cov(N_BURN)
    out = {"cov": pc.cov, "mean": pc.mean, "n": np.int64(pc.n)}
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
    np.savez(os.path.join(d_, "cov_w%d_rank%d.npz" % (world, rank)), **out)


if __name__ == "__main__":
    main()
