"""The contract every function compiled from a caller's source is installed under (csrc/sampler.hip: install_function): a source that does not
compile leaves the installed function whole -- its module, its parameters, its data and, for a pointwise density, the module of PSIS-LOO's stages
compiled around it.  8 chains x 5 generations of 2 coordinates, 3 data points of one value; the time is two or three run-time compilations."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _loo_cases as LC  # noqa: E402
import _waic_cases as WC  # noqa: E402

N, G, D, N_DATA = 8, 5, 2, 3
BROKEN = "__device__ double not_the_function(double a) { return a; }"


@pytest.fixture()
def eng():
    e = LC.installed(WC.make_history(G, N, D))
    yield e
    e.close()


def test_a_function_source_that_does_not_compile_leaves_the_installed_function_whole(eng):
    from bipymc_amd import HipFunction, _lib as L, derived as DV
    fn = HipFunction("__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {\n"
                     "    out[0] = x[0] * p[0]; out[1] = x[1] + p[1];\n}", n_out=2, params=[3.0, 0.25])
    before = DV.compute(eng.derive, DV.single_process_allgather, fn, 0, eng.n_chains, eng.history_rows(), values=True)
    assert before.values.shape == (N * G, 2)
    with pytest.raises(L.BpmError, match="bpm_set_device_function: the function source does not compile"):
        eng.set_device_function(BROKEN, 2, [1.0, 1.0])
    counts, sums, n, n_first, values = eng.derive_rows(0, values=True)          # (without reinstalling)
    assert n == N * G and n_first == 0
    assert np.array_equal(values, before.values)


def test_a_pointwise_source_that_does_not_compile_leaves_the_function_and_its_loo_module_whole(eng):
    from bipymc_amd import _lib as L
    pw = WC.pointwise(1, WC.make_data(N_DATA, 1))
    before = LC.waic(eng, pw, 0)
    assert before.values.shape == (N * G, N_DATA)
    first = LC.loo(eng, pw, 0)
    assert first.stats["compiled"] == 1
    with pytest.raises(L.BpmError, match="bpm_set_pointwise: the pointwise source does not compile"):
        eng.set_pointwise(BROKEN, WC.make_data(N_DATA, 1, seed=1), [1.0])
    values = eng.pointwise_rows(0, values=True)[4]                               # (without reinstalling)
    assert np.array_equal(values, before.values)
    again = LC.loo(eng, pw, 0)
    assert again.stats["compiled"] == 0                                          # the module of stages A and B was kept
    assert np.array_equal(again.elpd_loo_i, first.elpd_loo_i, equal_nan=True)
