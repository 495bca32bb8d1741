"""Child process of tests/test_gpu_nonfinite.py::test_alternative_kernel_paths_from_overflow_rows: three of the shipped-target cases from two start
rows of magnitude 1e160, 10 generations each, on whatever kernel path the environment selects (BPM_TEST_PATHS with the test variant of the library,
BPM_DIRECT_QUEUE); everything the run leaves is saved for a bit-for-bit comparison with the default path's.
usage: _nonfinite_worker.py <out.npz>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

GENS = 10


def cases():
    from bipymc_amd import _lib as L
    from bipymc_amd.utils import banana_rv, d100_gauss, mixture_nd
    # (DREAM without CR adaptation, as everywhere from these starts: tests/_nonfinite_cases.py, section 2)
    return (("dream_gauss100", d100_gauss.Gauss_100D()._bpm_target_spec(), L.ALGO_DREAM, 96, dict(burnin_gen=0)),
            ("dream_mix8", mixture_nd.BimodeGauss_ND(8)._bpm_target_spec(), L.ALGO_DREAM, 101, dict(burnin_gen=0, del_pairs=2)),
            ("demc_banana", banana_rv.Banana_2D()._bpm_target_spec(), L.ALGO_DEMC, 77, dict(p_snooker=0.2)))


def main():
    from _nonfinite_cases import overflow_rows
    from bipymc_amd.engine import HipEngine
    out = {}
    for name, (tid, tp, d), algo, N, kw in cases():
        e = HipEngine(algo=algo, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=5, **kw)
        e.set_state(overflow_rows(np.random.RandomState(0).normal(size=(N, d)) + 1.0))
        e.begin_run()
        e.step(GENS)
        st = e.stats()
        out[name + "_state"] = e.get_state()
        out[name + "_ll"] = e.get_loglike()
        out[name + "_ll_history"] = e.get_loglike_history()
        out[name + "_counts"] = np.array([st["local_n_accepted"], st["local_n_rejected"], st["n_nan_alpha"]], dtype=np.int64)
        e.close()
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
