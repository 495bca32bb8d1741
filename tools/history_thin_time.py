#!/usr/bin/env python3
"""Thinned histories at cfg2's shape (DREAM, 8192 chains x the 100-D Gaussian):
  (a) the steady-state generation with thin = 1, 2 and 10: bpm_step_timed over REPS calls of GENS generations each (device time between two
      update launches: the last three quarters of a call's launches), median, in us per generation -- a skipped generation appends no
      history row, 808 of the 7216 algorithmic bytes of an update;
  (b) thin_history(4) on a 1000-generation dense history, host-to-host, median of 3 fresh histories: the call gathers (rows - 1) // 4 + 1 rows
      into new buffers and returns the old ones; bytes = new rows x n_local x (ld + 1) x 8, read once and written once.
  (c) --headline PARENT.jsonl THIS.jsonl: the JSON lines of `python bench.py` (unchanged) on the parent commit and on this tree, the same
      number of runs each: median against median, and whether the difference lies inside the parent's own run-to-run spread.
The record goes to profiles/history_thin_cfg2.txt.
usage: history_thin_time.py [--out FILE] [--headline PARENT.jsonl THIS.jsonl] [--headline-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _history_bench import PEAK_BW, Report  # noqa: E402

N, BURNIN, WARM, GENS, REPS = 8192, 100, 150, 400, 5


def engine(thin):
    from bipymc_amd import _lib as L
    from bipymc_amd.engine import HipEngine
    from bipymc_amd.utils import d100_gauss
    tid, tp, d = d100_gauss.Gauss_100D()._bpm_target_spec()
    e = HipEngine(algo=L.ALGO_DREAM, n_chains=N, dim=d, target_id=tid, target_params=tp, seed=1, burnin_gen=BURNIN, n_cr_gen=20, thin=thin)
    e.set_state(np.random.RandomState(0).normal(size=(N, d)) * np.sqrt(np.arange(d) + 1.0))
    e.begin_run()
    return e, d


def generation_times(say):
    say("# (a) steady-state generation, bpm_step_timed, %d calls of %d generations after %d generations (burn-in %d); us per generation" % (REPS, GENS, WARM, BURNIN))
    base = None
    for thin in (1, 2, 10):
        e, d = engine(thin)
        e.reserve_history((WARM + GENS * REPS) // thin + 2)
        e.step(WARM)
        e.synchronize()
        us = []
        for _ in range(REPS):
            ms, n = e.step_timed(GENS)
            us.append(ms * 1e3 / n * 2.0)             # two update launches per generation
        rows = e.history_thin()["rows"]
        e.close()
        med = float(np.median(us))
        base = med if base is None else base
        say("thin = %2d: median %.3f us (min %.3f, max %.3f); %.4f of thin = 1; %d rows stored = %.2f GB"
            % (thin, med, min(us), max(us), med / base, rows, rows * N * (d + 1) * 8 / 1e9))


def thin_call_time(say):
    G, m = 1000, 4
    ts, moved = [], 0
    for _ in range(3):
        e, d = engine(1)
        e.step(G)
        e.synchronize()
        ld = d + (d & 1)
        t0 = time.perf_counter()
        e.thin_history(m)
        ts.append(time.perf_counter() - t0)
        rows = e.history_thin()["rows"]
        moved = rows * N * (ld + 1) * 8
        e.close()
    t = float(np.median(ts))
    say("# (b) thin_history(%d) on a %d-generation history (%d -> %d rows), host-to-host, median of 3 (min %.3f ms, max %.3f ms)" % (m, G, G + 1, rows, min(ts) * 1e3, max(ts) * 1e3))
    say("%.3f ms; reads %.3f GB and writes %.3f GB once: %.2f TB/s read + written = %.3f of 8 TB/s (the call also allocates the new buffers, "
        "waits for the stream and frees %.2f GB)" % (t * 1e3, moved / 1e9, moved / 1e9, 2 * moved / t / 1e12, 2 * moved / t / PEAK_BW, (G + 1) * N * (ld + 1) * 8 / 1e9))


def headline(say, parent_file, this_file):
    def values(path):
        out = []
        with open(path) as f:
            for line in f:
                line = line.strip()
                if line.startswith("{"):
                    out.append(float(json.loads(line)["value"]))
        return out
    p, t = values(parent_file), values(this_file)
    say("# (c) headline, python bench.py (unchanged), chain-updates/s, runs alternating in one session on one MI355X")
    say("parent n=%d: %s" % (len(p), " ".join("%.4e" % v for v in p)))
    say("this   n=%d: %s" % (len(t), " ".join("%.4e" % v for v in t)))
    if len(p) != len(t) or not p:
        say("NOT COMPARABLE: the two sets must have the same number of runs")
        return
    mp, mt = float(np.median(p)), float(np.median(t))
    say("parent median %.4e, min %.4e, max %.4e (spread %.2f %%); this median %.4e, min %.4e, max %.4e (spread %.2f %%)"
        % (mp, min(p), max(p), (max(p) - min(p)) / mp * 100, mt, min(t), max(t), (max(t) - min(t)) / mt * 100))
    inside = min(p) <= mt <= max(p)
    say("this median / parent median = %.4f; this median lies %s the parent's own runs [%.4e, %.4e]%s"
        % (mt / mp, "INSIDE" if inside else "OUTSIDE", min(p), max(p), "" if inside else (": ABOVE them" if mt > max(p) else ": BELOW them")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--headline", nargs=2, default=None, metavar=("PARENT", "THIS"))
    ap.add_argument("--headline-only", action="store_true")
    a = ap.parse_args()
    r = Report()
    if not a.headline_only:
        from bipymc_amd import _lib as L
        r.say("Thinned histories at cfg2's shape (tools/history_thin_time.py); library build id %s" % L.build_id(L.load()))
        generation_times(r.say)
        thin_call_time(r.say)
    if a.headline:
        headline(r.say, *a.headline)
    if a.out and a.headline_only and os.path.exists(a.out):      # (the headline runs are appended to the record of (a) and (b))
        with open(a.out) as f:
            r.lines = f.read().rstrip("\n").split("\n") + r.lines
    r.write(a.out)


if __name__ == "__main__":
    main()
