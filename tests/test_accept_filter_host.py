"""The accept test's decision logic (bipymc_amd/csrc/accept_test.h) in its host flavour -- exp2f in place of the device's v_exp_f32 -- against the
plain formula (exp, fmin, fmax, compare), in a stand-alone C++ program: tests/accept_filter_host_main.cpp.  No GPU.

Inputs: d in {+-0, +-1e-300, D_LO and its two neighbours, -745, -746, -1e300, +-inf, NaN} and 10^6 random values in [-45, 1]; u in {0, 2^-53,
1 - 2^-53}, random 53-bit values, and the five doubles within +-2 ulp of the clamped exp(d).  Every decision and every NaN flag must be the plain
formula's; the adversarial u must reach the exact path in some cases (they sit inside the filter's margin) and not in all (d >= 0 needs no exp)."""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("accept") / "accept_filter_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "bipymc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "accept_filter_host_main.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    print(out)
    rows = {}
    for line in out.splitlines():
        if line.startswith("#"):
            continue
        f = line.split()
        rows[f[0]] = [int(f[1])] + [int(x) for x in f[3::2]]
    return rows


def test_every_decision_and_nan_flag_is_the_plain_formulas(counts):
    for key in ("n_random_u", "n_adversarial"):
        n, diff_accept, diff_nan, _ = counts[key]
        assert n > 4000000 and diff_accept == 0 and diff_nan == 0, (key, counts[key])


def test_adversarial_u_reaches_the_exact_path_sometimes_not_always(counts):
    n, _, _, exact = counts["n_adversarial"]
    assert 0 < exact < n, counts["n_adversarial"]
    n, _, _, exact = counts["n_random_u"]
    assert 0 < exact < n // 10, counts["n_random_u"]      # (u = 0 below D_LO asks; a random u asks with probability <= 2 DELTA)


def test_exp_of_d_lo_is_below_the_smallest_nonzero_uniform(counts):
    assert counts["exp_d_lo_below_u_min"] == [1]
