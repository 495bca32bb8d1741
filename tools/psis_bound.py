#!/usr/bin/env python3
"""The gate of the PSIS tests, measured (no GPU): per quantity -- pareto_k, sigma (relative), the smoothed tail's log weights, elpd_loo_i --
the largest error of the float64 NumPy restatement of the statistic (tests/_psis_restatement.py) against the same statistic in mpmath at 200
bits on the cases of host_cases(), the error of bipymc_amd/csrc/psis.h on the same cases (tests/psis_host_main.cpp, built with the host
compiler), and the gate the tests allow the C++ and the device: 4 x the former -- a factor 2 for the device's exp and log at E = 2 ulp
(profiles/waic_bound.txt) against libm's 1, a factor 2 for another, but fixed, order of summation.

    python tools/psis_bound.py [OUT]     # default OUT: profiles/psis_bound.txt"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _psis_restatement as PR  # noqa: E402
import test_psis_host as TH  # noqa: E402


def main(argv):
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "psis_bound.txt")
    cases = PR.host_cases()
    exact = [PR.case_exact(c) for c in cases]
    ref = np.array([PR.errors(PR.fit_from_tail(c[1], c[2], c[3] + np.log(c[4])), e) for c, e in zip(cases, exact)])
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "psis_host")
        TH.build(exe, False)
        got = [TH.parse_tail(line) for line in TH.run(exe, [TH.tail_command(*c[1:]) for c in cases], os.path.join(td, "commands.txt"))]
    cpp = np.array([PR.errors(g, e) for g, e in zip(got, exact)])
    lines = ["# PSIS per datum against mpmath at 200 bits (tools/psis_bound.py): %d cases (tests/_psis_restatement.py: host_cases), tails of %s values"
             % (len(cases), ", ".join(str(e["tail_len"]) for e in exact)),
             "# quantity: the NumPy restatement's largest error | csrc/psis.h on the host | the tests' gate = 4 x the first"]
    for q, name in enumerate(TH.QUANTITIES):
        lines.append("%-18s %.3e (%s) | %.3e (%s) | %.3e" % (name, ref[:, q].max(), cases[int(np.argmax(ref[:, q]))][0], cpp[:, q].max(),
                                                            cases[int(np.argmax(cpp[:, q]))][0], 4 * ref[:, q].max()))
    lines.append("# errors are absolute, sigma's relative, elpd's relative to max(1, |elpd|).  tests/test_psis_host.py measures the first column again and allows psis.h on the")
    lines.append("# host 4 x it; the GPU tests read the gate from this file and hold stage C to it on its own inputs (tests/_loo_cases.py: check_fit)")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1:])
