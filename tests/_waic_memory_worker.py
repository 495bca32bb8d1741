"""The child process of tests/test_gpu_waic.py::test_a_closed_sampler_has_given_its_data_back:

    python tests/_waic_memory_worker.py OUT.txt

writes the free device memory after minus before a case that creates a sampler, installs a pointwise function with 4 MiB of data, reduces
and closes (tests/_memory_cases.py: measure -- one run as a warm-up, then the two readings)."""
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
    pw = WC.pointwise(1, np.linspace(-1.0, 1.0, 1 << 19))          # 4 MiB of data, 2048 data tiles
    res = MC._over(e).param_est_waic(pw, 3)
    assert res.n == MC.G * MC.N - 3 and np.isfinite(res.elpd_waic)
    e.set_pointwise(pw.source, pw.data[:1000], pw.params)             # replaced: the first copy goes here, the second with the handle
    e.close()


if __name__ == "__main__":
    diff = MC.measure(_case)
    print("pointwise", diff, flush=True)
    with open(sys.argv[1], "w") as f:
        f.write("%d\n" % diff)
