"""The steady-state and burn-in update kernels of one wavefront per chain with plan records (kernels.h: phase_fused_kernel, HOT = 1 / 3) order their
work around the arrival of the partner rows: row loads that every lane issues (load_row_all), the accept uniform and the gamma / jump selects ahead of
the row wait, the two likelihood sums reduced step by step together (gsum2), the history row stored first.  None of it may change a bit.

Reference: the general instantiation (BPM_TEST_PATHS=nohot, the test variant of the library), which shares the device functions but none of the
specialisation, and the same kernels launched on the HIP stream instead of the library's own queue.  State, ln-likes, the whole history with its
ln-likes and the accept counts must be EQUAL (np.array_equal), after 10 burn-in generations (n_cr_gen = 2: the CR statistics run from generation 3)
and 40 steady-state ones.

Shapes (d = 100 unless said, del_pairs = 3): N = 64 (two full 32-chain halves); N = 66 (halves of 33: the last two-wavefront workgroup of a launch is
half idle, the last 16-wavefront one of the burn-in kernel mostly); d = 99 (odd: ld = 100, the last lane's second coordinate is padding); d = 126
(63 lanes of pairs: header and pair lanes no longer fit beside them, the non-merged draw path of the general kernel; lane 63 holds no coordinate).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = (("n64", 64, 100), ("n66", 66, 100), ("d99", 64, 99), ("d126", 64, 126))
BURNIN, STEADY = 10, 40


def _run_case(N, d, direct):
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, dd = d100_gauss.Gauss_100D(dim=d)._bpm_target_spec()
    assert dd == d
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=17, del_pairs=3, burnin_gen=BURNIN, n_cr_gen=2)
    if direct is not None:
        assert e.launch_stats()["has_queue"], e.launch_stats()
        e.set_launch_path(direct, -1)
    e.set_state(np.random.RandomState(5).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0))
    e.begin_run()
    before = e.launch_stats()
    e.step(BURNIN)
    e.step(STEADY)
    after = e.launch_stats()
    if direct is not None:
        moved, still = ("direct", "stream") if direct else ("stream", "direct")
        assert after[moved] - before[moved] == 2 * (BURNIN + STEADY) and after[still] == before[still], (before, after)
    st = e.stats()
    out = dict(state=e.get_state(), ll=e.get_loglike(), hist=e.get_history(), llhist=e.get_loglike_history(),
               acc=np.array([st["local_n_accepted"], st["local_n_rejected"]], dtype=np.int64), p_cr=np.asarray(st["p_cr"]))
    e.close()
    return out


_CHILD = r'''
import os, sys, numpy as np
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_wave_tail as T
res = {}
for name, N, d in T.CASES:
    for k, v in T._run_case(N, d, None).items():
        res[name + "_" + k] = v
np.savez(sys.argv[1], **res)
'''


@pytest.fixture(scope="module")
def general_kernel():
    """Every case on the general instantiation (nohot), in ONE child process: the switch is read once per process, by the test variant only."""
    from bipymc_amd import _lib as L
    assert os.path.exists(L.TEST_LIB_PATH), "build_variants/libbipymc_test.so missing: make -C bipymc_amd/csrc"
    env = dict(os.environ)
    for k in ("BPM_DIRECT_QUEUE", "BPM_QUEUE_INFLIGHT"):
        env.pop(k, None)
    env["BPM_TEST_PATHS"] = "nohot"
    env["BPM_LIB_PATH"] = L.TEST_LIB_PATH
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "o.npz")
        subprocess.check_call([sys.executable, "-c", _CHILD, f], env=env, cwd=os.path.join(os.path.dirname(__file__), ".."))
        with np.load(f) as z:
            return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name,N,d", CASES, ids=[c[0] for c in CASES])
def test_hot_kernels_equal_the_general_kernel_and_the_stream_path_bit_for_bit(general_kernel, name, N, d):
    hot = _run_case(N, d, True)            # the shipped path: own queue, HOT = 3 in burn-in, HOT = 1 behind it
    stream = _run_case(N, d, False)        # the same kernels launched on the HIP stream
    assert hot["hist"].shape[0] >= BURNIN + STEADY and hot["hist"].shape[1:] == (N, d) and np.all(np.isfinite(hot["hist"]))
    assert 0 < hot["acc"][0] < N * (BURNIN + STEADY)
    for k in ("state", "ll", "hist", "llhist", "acc", "p_cr"):
        assert np.array_equal(hot[k], general_kernel[name + "_" + k]), (name, k, "HOT != general kernel")
        assert np.array_equal(hot[k], stream[k]), (name, k, "own queue != HIP stream")
