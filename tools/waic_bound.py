#!/usr/bin/env python3
"""The one constant of the WAIC tests' error bound that cannot be derived: E, the error in ulps of the device's double exp and log
(tests/_waic_cases.py).  Measured WITHOUT the pointwise kernel: a HipFunction returning exp(x[0]) and log(x[1]) through
param_est_fn(values=True) over an installed history that holds the arguments, against mpmath at 200 bits.

    python tools/waic_bound.py [OUT.txt]          (default profiles/waic_bound.txt)

Arguments: exp on [-708, 0] (what the online log-sum-exp feeds it: l - m <= 0; below -708 the result is subnormal or 0 and its absolute
error is below 2^-1074), half of them in [-1, 0]; log on [1, 2^40] log-uniformly (s >= 1: the running sum counts its maximum as 1), half of
them in [1, 2].  A finite sample cannot show the worst case: the tests use twice the largest error seen."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SRC = """
__device__ void derive(const double* x, int d, double ll, const double* p, double* out) {
    out[0] = exp(x[0]);
    out[1] = log(x[1]);
}"""


def ulps(got, exact):
    """|got - exact| in units of the last place of exact (mpmath numbers in, float out)"""
    import mpmath as mp
    e = int(mp.floor(mp.log(abs(exact), 2)))
    return float(abs(mp.mpf(got) - exact) / mp.mpf(2) ** (e - 52))


def main(out_path):
    import mpmath as mp
    from bipymc_amd import HipFunction
    from _history_cases import _engine, _over
    mp.mp.prec = 200
    N, G = 16, 4096
    rs = np.random.RandomState(11)
    X = np.empty((G, N, 2))
    a = rs.uniform(-708.0, 0.0, size=G * N)
    a[::2] = rs.uniform(-1.0, 0.0, size=G * N // 2)
    b = np.exp2(rs.uniform(0.0, 40.0, size=G * N))
    b[::2] = rs.uniform(1.0, 2.0, size=G * N // 2)
    X[:, :, 0], X[:, :, 1] = a.reshape(G, N), b.reshape(G, N)
    e = _engine(N, 2)
    e.set_history(X, X[-1])
    V = _over(e).param_est_fn(HipFunction(SRC, n_out=2), 0, values=True).values
    H = e.get_history().reshape(-1, 2)
    e.close()
    assert np.array_equal(H, X.reshape(-1, 2))
    worst = [0.0, 0.0]
    at = [0.0, 0.0]
    for r in range(len(H)):
        for k, f in ((0, mp.exp), (1, mp.log)):
            exact = f(mp.mpf(H[r, k]))
            if exact == 0:
                assert V[r, k] == 0.0
                continue
            u = ulps(V[r, k], exact)
            if u > worst[k]:
                worst[k], at[k] = u, float(H[r, k])
    seen = max(worst)
    lines = ["error of the device's double exp and log in ulps, %d arguments each, against mpmath at 200 bits" % len(H),
             "  (a HipFunction through param_est_fn(values=True): code of the commit before the pointwise kernel)",
             "exp on [-708, 0]:   largest error %.4f ulp at x = %r" % (worst[0], at[0]),
             "log on [1, 2^40]:   largest error %.4f ulp at x = %r" % (worst[1], at[1]),
             "largest seen: %.4f ulp; the tests use E = 2 x that, rounded up to a whole ulp: E = %d" % (seen, int(np.ceil(2.0 * seen)))]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "waic_bound.txt"))
