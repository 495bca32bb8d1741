"""One rank of a world of processes sharing one GPU for tests/test_gpu_diagnostics.py: DreamMpi over the push exchange, then the
collective convergence_diagnostics.  usage: _diag_worker.py <dir> <rank> <world>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(comm):
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.5, dim=10)
    s = DreamMpi(t.ln_like, np.zeros(10), n_chains=64, mpi_comm=comm, n_cr_gen=3, burnin_gen=10, seed=77,
                 exchange="push" if comm is not None else "auto")
    s.run_mcmc(64 * 60)
    res = s.convergence_diagnostics(n_burn=64 * 10 + 3)
    return {f: np.asarray(getattr(res, f)) for f in res._fields}


def main():
    d_, rank, world = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    comm = None
    if world > 1:
        from _file_comm import FileComm
        comm = FileComm(d_, rank, world)
    out = run(comm)
    np.savez(os.path.join(d_, "diag_w%d_rank%d.npz" % (world, rank)), **out)


if __name__ == "__main__":
    main()
