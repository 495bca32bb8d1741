"""The child process of tests/test_gpu_loo.py::test_a_closed_sampler_has_given_its_scratch_back:

    python tests/_loo_memory_worker.py OUT.txt

writes the free device memory after minus before a case that creates a sampler, runs param_est_loo over 2000 data (stage A's buffers, the
sort's temporaries, the fit's work space, the second run-time module) and closes (tests/_memory_cases.py: measure -- one run as a warm-up,
then the two readings)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _memory_cases as MC  # noqa: E402
import _waic_cases as WC  # noqa: E402


def _case():
    e, _X = MC._installed()
    pw = WC.pointwise(1, np.linspace(-1.0, 1.0, 2000))
    res = MC._over(e).param_est_loo(pw, 3, tails=True)
    assert res.n == MC.G * MC.N - 3 and np.isfinite(res.elpd_loo) and len(res.tails) == 2000
    e.close()


if __name__ == "__main__":
    diff = MC.measure(_case)
    print("loo", diff, flush=True)
    with open(sys.argv[1], "w") as f:
        f.write("%d\n" % diff)
