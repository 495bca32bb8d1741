#!/usr/bin/env python3
"""Bit-level fingerprints of the update kernels: a list of tiny samplers, one per kernel shape, each run for a few generations from a fixed
state; of every run the SHA-256 of the final state, the ln-likes, the whole history (rows and ln-likes), p_cr and the CR statistics, and the
accept counts.

    BPM_LIB_PATH=build_variants/libbipymc_<parent>.so BPM_ALLOW_STALE_LIB=1 python tools/update_bits.py --write     (on the GPU)

runs the list on the library BPM_LIB_PATH names (default: the tree's) and writes tests/golden/update_bits.json.  The file is taken ONCE, on the
library of the commit BEFORE a change that may only re-schedule the kernels' arithmetic (other lanes, other instructions, the same sums in the
same order); tests/test_gpu_update_bits.py runs the same list on the tree's library and compares the digests.  Without --write the digests are
printed and compared with the file."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "update_bits.json")

N_CHAINS, N_GENS = 128, 12
ALGO_DEMC, ALGO_DREAM = 0, 1
TARGET_GAUSS_EQUICORR = 1
ASSOC_SEED = 11          # the association-order case: seed of its start and of its sampler (tests/test_gpu_update_bits.py checks it on the CPU)


def gauss_params(d):
    """oracle/sampler_ref.py: gauss_equicorr_params(0.5, sqrt(1 .. d)) -- restated here, tools do not import the oracle"""
    sigma = np.sqrt(np.arange(d) + 1.0)
    rho = 0.5
    logdet = 2.0 * np.sum(np.log(sigma)) + (d - 1) * np.log(1.0 - rho) + np.log(1.0 + (d - 1) * rho)
    c0 = -0.5 * (d * np.log(2.0 * np.pi) + logdet)
    return np.concatenate([[rho, c0, 1.0 / (1.0 - rho), rho / ((1.0 + (d - 1) * rho) * (1.0 - rho))], 1.0 / sigma])


def start_state(d, seed):
    return np.random.RandomState(seed).normal(size=(N_CHAINS, d)) * np.sqrt(np.arange(d) + 1.0)


def assoc_state(d, seed):
    """Coordinates 0, 2, 4, ... alternate +1e8, -1e8 (plus a value of order 1), coordinates 1, 3, 5, ... are of order 1: sum z cancels from 1e8 down to
    order 1 and sum z^2 carries 1e16 next to order 1, so both change in their last bits under ANY other association of the additions."""
    X = np.random.RandomState(seed).normal(size=(N_CHAINS, d))
    big = np.zeros(d)
    big[0::4] = 1e8
    big[2::4] = -1e8
    return X + big[None, :]


def cases():
    """-> [(name, algo, d, engine keywords, start state)]"""
    out = []
    for d in (100, 34, 127, 32, 8, 2):
        out.append(("dream_adapt_d%d" % d, ALGO_DREAM, d, dict(burnin_gen=1 << 20, n_cr_gen=4, seed=100 + d), start_state(d, d)))
        out.append(("dream_steady_d%d" % d, ALGO_DREAM, d, dict(burnin_gen=0, seed=200 + d), start_state(d, d + 1)))
    for d in (100, 2):
        out.append(("demc_snooker_d%d" % d, ALGO_DEMC, d, dict(p_snooker=0.1, seed=300 + d), start_state(d, d + 2)))
    out.append(("dream_steady_wide_d640", ALGO_DREAM, 640, dict(burnin_gen=0, seed=840), start_state(640, 642)))
    out.append(("dream_steady_d100_association", ALGO_DREAM, 100, dict(burnin_gen=0, seed=ASSOC_SEED), assoc_state(100, ASSOC_SEED)))
    return out


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(algo, d, kw, X0, lib=None):
    from bipymc_amd.engine import HipEngine
    eng = HipEngine(algo=algo, n_chains=N_CHAINS, dim=d, target_id=TARGET_GAUSS_EQUICORR, target_params=gauss_params(d), lib=lib, **kw)
    try:
        eng.set_state(X0)
        eng.begin_run()
        eng.step(N_GENS)
        st = eng.stats()
        return dict(state=_sha(eng.get_state()), loglike=_sha(eng.get_loglike()), history=_sha(eng.get_history()),
                    loglike_history=_sha(eng.get_loglike_history()), history_rows=int(st["history_rows"]),
                    p_cr=_sha(np.asarray(st["p_cr"], dtype=np.float64)), delta_m=_sha(np.asarray(st["delta_m"], dtype=np.float64)),
                    n_cr_updates=_sha(np.asarray(st["n_cr_updates"], dtype=np.float64)),
                    n_accepted=int(st["local_n_accepted"]), n_rejected=int(st["local_n_rejected"]), n_nan_alpha=int(st["n_nan_alpha"]))
    finally:
        eng.close()


def run_all(lib=None):
    return {name: run_case(algo, d, kw, X0, lib) for name, algo, d, kw, X0 in cases()}


if __name__ == "__main__":
    from bipymc_amd import _lib
    got = run_all()
    doc = dict(library_build_id=_lib.build_id(_lib.load()), n_chains=N_CHAINS, n_gens=N_GENS, cases=got)
    if "--write" in sys.argv:
        rest = sys.argv[sys.argv.index("--write") + 1:]
        GOLDEN = rest[0] if rest else GOLDEN          # --write [FILE]: somewhere else than the tree
        with open(GOLDEN, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote %s from library %s: %d cases" % (GOLDEN, doc["library_build_id"], len(got)))
    else:
        with open(GOLDEN) as f:
            want = json.load(f)
        bad = [k for k in want["cases"] if got.get(k) != want["cases"][k]]
        for k in sorted(got):
            print("%-34s %s  accepted %d" % (k, "DIFFERS" if k in bad else "same bits", got[k]["n_accepted"]))
        print("library %s against the file's %s: %d of %d cases differ" % (doc["library_build_id"], want["library_build_id"], len(bad), len(want["cases"])))
        sys.exit(1 if bad else 0)
