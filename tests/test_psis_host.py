"""The plain-C++ part of bipymc_amd/csrc/psis.h on the host (tests/psis_host_main.cpp), against the two restatements of
tests/_psis_restatement.py: the kept-set size, the tie rule, the rule for tails of 4 or fewer, and k, sigma, the smoothed tail and elpd_loo_i
of the cases of host_cases() against mpmath at 200 bits.

THE GATE is not a tuned number: per quantity it is 4 x the largest error of the float64 NumPy restatement against the same mpmath reference on
the same cases -- a factor 2 for the device's exp and log at E = 2 ulp (profiles/waic_bound.txt) against libm's 1, a factor 2 for another
(fixed) order of summation.  tools/psis_bound.py writes both sets of numbers to profiles/psis_bound.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _psis_restatement as PR  # noqa: E402

QUANTITIES = PR.QUANTITIES


def build(exe, sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + flags + ["-I", os.path.join(ROOT, "bipymc_amd", "csrc"),
                                                                                             os.path.join(HERE, "psis_host_main.cpp"), "-o", exe, "-ldl"])


def run(exe, commands, path):
    with open(path, "w") as f:
        f.write("\n".join(commands) + "\n")
    return subprocess.check_output([exe, path]).decode().splitlines()


def tail_command(tail, n_body, m_b, s_b):
    return "T %d %d %s %s %s" % (len(tail), n_body, float(m_b).hex(), float(s_b).hex(), " ".join(float(v).hex() for v in tail))


def parse_tail(line):
    f = line.split()
    assert f[0] == "T"
    n = int(f[4])
    return dict(k=float.fromhex(f[1]), sigma=float.fromhex(f[2]), elpd=float.fromhex(f[3]), tail_len=n,
                smoothed=np.array([float.fromhex(v) for v in f[5:5 + n]]))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("psis_host")
    plain, san = str(d / "psis_host"), str(d / "psis_host_san")
    build(plain, False)
    build(san, True)
    return plain, san, str(d / "commands.txt")


@pytest.fixture(scope="module")
def measured():
    """the cases, their exact results and the NumPy restatement's errors: computed once"""
    cases = PR.host_cases()
    exact = [PR.case_exact(c) for c in cases]
    infos = [dict() for _ in cases]
    mine = [PR.fit_from_tail(c[1], c[2], c[3] + np.log(c[4]), info=i) for c, i in zip(cases, infos)]
    errs = np.array([PR.errors(g, e) for g, e in zip(mine, exact)])
    return cases, exact, mine, errs, infos


def test_restatement_and_psis_h_recover_the_shape_of_exact_quantiles(programs):
    """the sanity check of the restatement, and the same of psis.h on the host: both see the same tails"""
    tails = [PR.tail_from_excesses(PR.gpd_quantiles(1000, k)) for k in (0.1, 0.5, 0.9)]
    out = run(programs[1], [tail_command(t, 4000, 0.0, 1.0) for t in tails], programs[2])
    for who, ks in (("the restatement", [PR.fit_from_tail(t, 4000, 0.0)["k"] for t in tails]), ("psis.h", [parse_tail(line)["k"] for line in out])):
        print("%s: k_hat of exact quantiles, n = 1000, true k 0.1, 0.5, 0.9:" % who, ks)
        assert ks[0] < ks[1] < ks[2], who
        for true, got in zip((0.1, 0.5, 0.9), ks):
            assert min(true, 0.5) - 0.002 <= got <= max(true, 0.5) + 0.002, (who, true, got)
    assert all(parse_tail(line)["tail_len"] == 1000 for line in out)


def test_cases_cover_what_they_claim(programs, measured):
    """in the restatement's results and in psis.h's own"""
    cases, exact, mine, errs, infos = measured
    cpp = [parse_tail(line) for line in run(programs[1], [tail_command(*c[1:]) for c in cases], programs[2])]
    for results in (mine, cpp):
        got = {c[0]: r for c, r in zip(cases, results)}
        for n in (5, 6, 29, 30, 31, 255, 256, 257):
            assert got["gpd draws n=%d" % n]["tail_len"] == n
        assert abs(got["exponential"]["k"]) < 0.15 and 0.9 < got["k=1.2"]["k"] < 1.3
        assert got["tail of 4"]["tail_len"] == 4 and got["tail of 4"]["k"] == np.inf
        assert got["tail of 0"]["tail_len"] == 0 and got["tail of 0"]["k"] == np.inf
        assert np.isfinite([r["elpd"] for r in results]).all()
    by = {c[0]: (m, i) for c, m, i in zip(cases, mine, infos)}
    for n in (5, 6, 29, 30, 31, 255, 256, 257):
        assert by["gpd draws n=%d" % n][0]["tail_len"] == n
    assert abs(by["exponential"][0]["k"]) < 0.15 and 0.9 < by["k=1.2"][0]["k"] < 1.3
    assert by["weights cut"][1]["dropped"] > 0 and by["gpd draws n=30"][1].get("dropped", 0) == 0
    assert by["tail of 4"][0]["tail_len"] == 4 and by["tail of 4"][0]["k"] == np.inf
    assert by["tail of 0"][0]["tail_len"] == 0 and by["tail of 0"][0]["k"] == np.inf
    assert np.isfinite([m["elpd"] for m in mine]).all()


@pytest.mark.parametrize("sanitized", [False, True])
def test_fit_smoothing_and_elpd_against_mpmath_within_four_times_numpys_own_error(programs, measured, sanitized):
    cases, exact, mine, errs, infos = measured
    out = run(programs[1 if sanitized else 0], [tail_command(*c[1:]) for c in cases], programs[2])
    assert len(out) == len(cases)
    got = [parse_tail(line) for line in out]
    cpp = np.array([PR.errors(g, e) for g, e in zip(got, exact)])
    ref = errs.max(axis=0)
    for q, name in enumerate(QUANTITIES):
        print("%-18s NumPy restatement: largest error %.3e; psis.h on the host: %.3e; gate %.3e" % (name, ref[q], cpp[:, q].max(), 4 * ref[q]))
    for q, name in enumerate(QUANTITIES):
        worst = int(np.argmax(cpp[:, q]))
        assert cpp[:, q].max() <= 4.0 * ref[q], (name, cases[worst][0], cpp[worst, q], 4.0 * ref[q])
    for g, e in zip(got, exact):
        assert g["tail_len"] == e["tail_len"]


def test_kept_set_size_on_the_host(programs):
    S = (1, 4, 5, 6, 20, 21, 224, 225, 226)
    cmds = ["K %d %s" % (s, float(r).hex()) for s in S for r in (1.0, 0.25)]
    out = run(programs[1], cmds, programs[2])
    got = [int(line.split()[1]) for line in out]
    want = [PR.kept(s, r) for s in S for r in (1.0, 0.25)]
    assert got == want
    # the numbers themselves, by hand: M = ceil(min(S / 5, 3 sqrt(S / r_eff))), K = min(M + 1, S)
    assert dict(zip([(s, r) for s in S for r in (1.0, 0.25)], got)) == {
        (1, 1.0): 1, (1, 0.25): 1, (4, 1.0): 2, (4, 0.25): 2, (5, 1.0): 2, (5, 0.25): 2, (6, 1.0): 3, (6, 0.25): 3, (20, 1.0): 5, (20, 0.25): 5,
        (21, 1.0): 6, (21, 0.25): 6, (224, 1.0): 46, (224, 0.25): 46, (225, 1.0): 46, (225, 0.25): 46, (226, 1.0): 47, (226, 0.25): 47}


def test_ties_with_the_cutoff_belong_to_the_body_and_short_tails_are_not_smoothed(programs):
    def one(tail, n_body):
        body = np.full(n_body, tail[-1])
        m_b = float(np.max(-body))
        line = run(programs[1], [tail_command(tail, n_body, m_b, float(np.sum(np.exp(-body - m_b))))], programs[2])[0]
        return parse_tail(line), PR.fit_from_tail(tail, n_body, m_b + np.log(float(n_body)))
    # 12 kept values of which the last 3 tie the cutoff: the tail has 9
    tail = np.concatenate([np.linspace(-9.0, -5.0, 9), [-4.0, -4.0, -4.0]])
    got, want = one(tail, 30)
    assert got["tail_len"] == 9 == want["tail_len"] and np.isfinite(got["k"])
    # all kept values equal: no tail at all; 5 kept values with 4 below the cutoff: k = +inf and the log weights are the ratios themselves
    got, _ = one(np.full(6, -3.0), 10)
    assert got["tail_len"] == 0 and got["k"] == np.inf
    tail = np.array([-8.0, -7.0, -6.5, -6.0, -5.0])
    got, want = one(tail, 20)
    assert got["tail_len"] == 4 and got["k"] == np.inf and np.isnan(got["sigma"])
    assert np.array_equal(got["smoothed"], (tail[0] - tail[:4])[::-1])
    # with nothing smoothed elpd_loo is the plain importance sampling estimate: log(S) - logsumexp(-l) over all S draws
    l = np.concatenate([tail[:4], np.full(20, tail[4])])
    plain = np.log(len(l)) - (np.max(-l) + np.log(np.sum(np.exp(-l - np.max(-l)))))
    assert abs(got["elpd"] - plain) <= 8 * np.finfo(float).eps * abs(plain)
    # 6 kept values, 5 below the cutoff: the smallest tail that is fitted
    got, want = one(np.array([-8.0, -7.0, -6.5, -6.0, -5.5, -5.0]), 20)
    assert got["tail_len"] == 5 and np.isfinite(got["k"]) and abs(got["k"] - want["k"]) < 1e-12
