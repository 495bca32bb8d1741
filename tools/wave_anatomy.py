#!/usr/bin/env python3
"""Diagnostic (never part of the product): where one wavefront of the steady-state DREAM update kernel spends its life at the
headline shape (100-D Gaussian, 8192 chains, del_pairs = 3, history kept), from the stamp build
(`make -C bipymc_amd/csrc stamps` -> build_variants/libbipymc_stamps.so, which times the HOT = 1 instantiation itself).

Stamps are s_memtime (shader cycles, per CU: only differences inside one wavefront mean anything) plus the device-wide 100 MHz
counter at entry (slot 2) and at the end (slot 7).  The stamp build's fences forbid overlaps the product kernel has: read the
SHARES, not the length.

    python tools/wave_anatomy.py [--chains 8192] [--gens 120] [--out FILE]      (BPM_LIB_PATH: another stamp build)
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bipymc_amd import _lib as L          # noqa: E402
L.LIB_PATH = os.environ.get("BPM_LIB_PATH") or os.path.join(ROOT, "build_variants", "libbipymc_stamps.so")
from bipymc_amd.engine import HipEngine   # noqa: E402
from bipymc_amd.utils import d100_gauss   # noqa: E402


def pct(x):
    return "median %7.0f  p90 %7.0f" % (np.median(x), np.percentile(x, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--gens", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s)
        lines.append(s)

    N = args.chains
    tid, tp, d = d100_gauss.Gauss_100D()._bpm_target_spec()
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=1, burnin_gen=0)
    lib = e.lib
    lib.bpm_debug_stamps.restype = C.c_int
    lib.bpm_debug_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    e.set_state(np.random.RandomState(0).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0))
    L.check(lib.bpm_debug_stamps(e._h, None, 0))        # allocate: every launch stamps, the buffer keeps the last one's
    e.begin_run()
    e.step(args.gens)                                   # untimed: steady state, history kept
    n = N // 2
    out = np.zeros((n, 8), dtype=np.uint64)
    L.check(lib.bpm_debug_stamps(e._h, out.ctypes.data_as(C.c_void_p), n))
    say("wave anatomy: DREAM 100-D Gaussian, N=%d, del_pairs=3, steady state behind %d generations; build id %s (stamp build)"
        % (N, args.gens - 1, L.build_id(lib)))
    xcc = (out[:, 7] >> np.uint64(60)).astype(np.int64)
    rt0 = out[:, 2].astype(np.int64)
    rt1 = (out[:, 7] & np.uint64(0x0FFFFFFFFFFFFFFF)).astype(np.int64)
    ok = (out[:, 6] > 0) & (rt0 > 0)
    last = ok & (rt0 >= rt0[ok].max() - 3000)           # the last launch only (the buffer is reused by every launch)
    t = out.astype(np.float64)[last]
    r0, r1, xc = rt0[last], rt1[last], xcc[last]
    say("last launch: %d of %d wavefronts (second half generation)" % (last.sum(), n))
    # the shader clock from the two counters, over the wavefronts' lifetimes
    cyc, ns = t[:, 6] - t[:, 0], (r1 - r0) * 10.0
    mhz = np.median(cyc[ns > 0] / ns[ns > 0]) * 1e3
    say("shader clock (median of s_memtime / 100 MHz counter over wavefront lifetimes): %.0f MHz" % mhz)
    say("per wavefront, shader cycles (s_memtime):")
    # (a build whose planned front requests the rows first stamps "rows requested" AHEAD of slot 3 -- the header words are read out of the record behind
    # the row requests and the wait for everything else -- so there the second line is negative and the first one reads "entry -> all scalars in")
    seg = [("entry -> rows requested (slot 1 <- 7)", 0, 1),
           ("entry -> record in hand (slot 3)", 0, 3), ("record in hand -> rows requested (slot 1 <- 7)", 3, 1),
           ("rows requested -> proposal built: rows in (slot 4)", 1, 4), ("proposal built -> proposal ln-like done (slot 5)", 4, 5),
           ("ln-like done -> end of finish_update (slot 6)", 5, 6), ("rows requested -> end of finish_update", 1, 6),
           ("entry -> end of finish_update", 0, 6)]
    for name, i0, i1 in seg:
        dt = t[:, i1] - t[:, i0]
        say("   %-52s %s cycles  (%5.2f us median)" % (name, pct(dt), np.median(dt) / mhz))
    life = (r1 - r0) * 10.0
    say("   %-52s %s ns" % ("entry -> wave end (device-wide counter, 10 ns ticks)", pct(life)))
    o0, o1 = (r0 - r0.min()) * 10.0, (r1 - r0.min()) * 10.0
    say("launch, device-wide counter, ns after the first wavefront's start:")
    say("   wavefront starts (the ramp): p10 %5.0f  p50 %5.0f  p90 %5.0f  max %5.0f" % (np.percentile(o0, 10), np.percentile(o0, 50), np.percentile(o0, 90), o0.max()))
    say("   wavefront ends:              p10 %5.0f  p50 %5.0f  p90 %5.0f  max %5.0f" % (np.percentile(o1, 10), np.percentile(o1, 50), np.percentile(o1, 90), o1.max()))
    for x in range(8):
        sx = xc == x
        if sx.sum():
            say("   xcd %d: %5d wavefronts, starts %5.0f..%5.0f, ends %5.0f..%5.0f" % (x, sx.sum(), o0[sx].min(), o0[sx].max(), o1[sx].min(), o1[sx].max()))
    e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
