"""One rank of a world of processes sharing one GPU for tests/test_gpu_traces.py: DreamMpi over the push exchange, then the collective
param_est_trace of the history (and, in a one-rank world, the history and log-likelihoods NumPy's answer is taken over).
usage: _trace_worker.py <dir> <rank> <world>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

N, DIM, GENS = 64, 10, 60
N_BURN = N * 10 + 3
KW = dict(every=7, chains=[63, 0, 33, 5])      # chains of both ranks of a two-rank world


def run(comm):
    from bipymc_amd import DreamMpi
    from bipymc_amd.utils import d100_gauss
    t = d100_gauss.Gauss_100D(rho=0.5, dim=DIM)
    s = DreamMpi(t.ln_like, np.zeros(DIM), n_chains=N, mpi_comm=comm, n_cr_gen=3, burnin_gen=10, seed=77,
                 exchange="push" if comm is not None else "auto")
    s.run_mcmc(N * GENS)
    pt = s.param_est_trace(N_BURN, **KW)
    out = {f: np.asarray(getattr(pt, f)) for f in pt._fields}
    if comm is None:
        out["history"] = s._engine.get_history()
        out["loglike_history"] = s._engine.get_loglike_history()
    return out


def main():
    d_, rank, world = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    comm = None
    if world > 1:
        from _file_comm import FileComm
        comm = FileComm(d_, rank, world)
    np.savez(os.path.join(d_, "tr_w%d_rank%d.npz" % (world, rank)), **run(comm))


if __name__ == "__main__":
    main()
