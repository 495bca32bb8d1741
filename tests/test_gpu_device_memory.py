"""The sampler's device memory has one owner (bipymc_amd/csrc/device_memory.h: MemRegistry, DevTemp): nothing is lost, nothing changes.

NOTHING IS LOST.  Every case of tests/_memory_cases.py creates, runs and closes a sampler; between them they take every allocation branch
of bpm_create, every buffer that grows, and the second handle of derived_history / rank_history.  A case runs once as a warm-up, then
between two readings of the free device memory (hipMemGetInfo): a buffer that the registry does not know, or an old buffer that a regrow
does not release, is a difference.  The two readings must be EQUAL.  How they are taken (_memory_cases.measure):
  - In ONE child process with HSA_DISABLE_FRAGMENT_ALLOCATOR=1.  By default the HSA runtime serves allocations below 2 MiB from 2 MiB
    blocks of its own, and a lost buffer of these small cases does not move the free memory at all; without that allocator every
    allocation is the device's own, 2 MiB at the least, and every lost buffer shows.
  - The driver gives a closed sampler's memory back asynchronously, within some tens of milliseconds of bpm_destroy's return (on the parent
    commit as on this one; readings taken at once differ by a few to 28 MiB in either direction now and then, readings taken 50 ms later
    never did).  So the first reading is taken once the warm-up's memory has stopped moving, and the second is repeated, back to back, until
    it equals the first or two seconds have passed: memory on its way back arrives, memory that is lost does not.

NOTHING CHANGES.  Where a buffer grows, the results before and after equal, bit for bit, those of a twin that had the capacity before the
first row was written -- as far as the library lets a caller say so: the history through reserve_history; the running sums by stepping all
generations in one call (the buffer then grows once, while it holds the start row only); the quantile scratch by making the larger request
first.  The outlier check's keys are sized by the check itself, and the autocovariance partials by the sampler's shape alone (allocated
once per handle, they never grow on it), so their twins can only repeat the run.  The second handle of derived_history / rank_history is
checked by the checkers of those statistics' own tests, fresh and filled again."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _memory_cases as MC  # noqa: E402

CHILD_LIMIT_S = 60


@pytest.fixture(scope="module")
def readings(tmp_path_factory):
    """every case's differences of the free device memory, from one child process without the runtime's fragment allocator"""
    out = str(tmp_path_factory.mktemp("memory") / "readings.json")
    env = dict(os.environ)
    env["HSA_DISABLE_FRAGMENT_ALLOCATOR"] = "1"
    subprocess.check_call(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(HERE, "_memory_cases.py"), out], env=env,
                          timeout=CHILD_LIMIT_S + 30)
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("case", MC.CREATE + MC.GROWS + MC.SECOND, ids=MC.name)
def test_a_closed_sampler_has_given_everything_back(readings, case):
    diff = readings[MC.name(case)]
    print("%s: free device memory after - before: %d bytes" % (MC.name(case), diff))
    assert diff == 0


@pytest.mark.parametrize("case", MC.GROWS, ids=MC.name)
def test_a_buffer_that_grows_changes_nothing(case):
    case(check=True)


@pytest.mark.parametrize("case", MC.SECOND, ids=MC.name)
def test_second_handle_fresh_and_filled_again(case):
    case(check=True)
