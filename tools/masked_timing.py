#!/usr/bin/env python3
"""Cost of the mask in the fused update (K5): one masked and one unmasked
session of the same problem on the same GPU, timed in alternating runs.

    python tools/masked_timing.py [--n 512] [--r 8] [--missing 0.15] [--iters 20] [--rounds 6]

The problem is synth.low_rank_plus_outliers(n, n, n, r) in fp64 with the
traffic opts (tol = 0, so nothing stops).  Each round runs `iters` iterations
on the unmasked session, then on the masked one, first with K5 between events
(TRITD_TIMING_K5) and then untimed for the wall-clock iteration time.  Both
sessions probe the placement of their tensor pool (TRITD_SESSION_PROBE), so
that both stream from a fast placement.  Prints one JSON line:
the median over the rounds of K5 ms for both, their ratio, and iteration ms.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "triple-tensor-decomposition-with-admm_amd"))

import tritd  # noqa: E402
from tritd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--r", type=int, default=8)
    ap.add_argument("--missing", type=float, default=0.15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    n, r = a.n, a.r
    d = synth.low_rank_plus_outliers(n, n, n, r)
    observed = np.asfortranarray(np.random.default_rng(7).random(d["D"].shape) >= a.missing)
    opts = dict(synth.TRAFFIC_OPTS, tol=0.0, maxIter=a.warmup + 2 * a.rounds * a.iters + 1)
    kw = dict(n1=n, n2=n, n3=n, D=d["D"], device=0, probe=True)
    sess = {"unmasked": tritd.Session(r, opts, d["A0"], d["B0"], d["C0"], **kw),
            "masked": tritd.Session(r, opts, d["A0"], d["B0"], d["C0"], observed=observed, **kw)}
    k5 = {k: [] for k in sess}
    it = {k: [] for k in sess}
    for s in sess.values():
        s.run(a.warmup)
        s.sync()
    for _ in range(a.rounds):
        for name, s in sess.items():
            s.set_timing("k5")
            s.run(a.iters)
            s.sync()
            k5[name].append(s.kernel_ms()["fused_update"])
            s.set_timing(0)
            t0 = time.perf_counter()
            s.run(a.iters)
            s.sync()
            it[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = dict(shape=[n, n, n], r=r, missing=a.missing, iters=a.iters, rounds=a.rounds,
               observed=int(sess["masked"].mask_info()[1]))
    for name in sess:
        out["k5_ms_" + name] = round(statistics.median(k5[name]), 5)
        out["k5_ms_" + name + "_min_max"] = [round(min(k5[name]), 5), round(max(k5[name]), 5)]
        out["iter_ms_" + name] = round(statistics.median(it[name]), 5)
        out["probe_ms_" + name] = round(min(sess[name].probe()[0]), 4)
    out["k5_ratio"] = round(out["k5_ms_masked"] / out["k5_ms_unmasked"], 5)
    out["iter_ratio"] = round(out["iter_ms_masked"] / out["iter_ms_unmasked"], 5)
    for s in sess.values():
        s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
