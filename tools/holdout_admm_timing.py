#!/usr/bin/env python3
"""Cost of the held-out scores of the masked ADMM: one holdout and one masked
Session of the same fit on the same GPU, timed in alternating runs.

    python tools/holdout_admm_timing.py [--n 512] [--r 8] [--missing 0.15] [--holdout 0.10]
                                        [--iters 20] [--rounds 6] [--no-probe] [--holdout-first]
                                        [--out profiles/holdout_admm/holdout_admm_timing.json]

The problem is synth.low_rank_plus_outliers(n, n, n, r) in fp64 with the
traffic options, tol = 0 and patience = 0 (nothing stops).  `missing` of the
entries are unobserved and `holdout` of the observed ones are held out; the
masked session (the yardstick: the code path as it was before holdout existed)
gets observed = Omega & ~H, so both fit the same entries, and K5 is the same
code object in both.  Each round runs `iters` iterations on the masked
session, then on the holdout one, first with events around the iteration, K2,
K5 and (holdout) the score kernel (set_timing) and then untimed for the
wall-clock iteration time.  A holdout iteration ends with the score kernel (it
reads T, N x 8 B, the compact held-out values and 32 B of words and 8 B of
offset per tile), its pair reduction, the reduction of K5's norm partials, the
one-thread finish and the snapshot kernel, instead of leaving the norms to an
extra workgroup of the next M1.  Prints one JSON line (and writes it to
--out): medians over the rounds with min-max of K5 ms and iteration ms for
both, the score kernel's ms and achieved bandwidth, the tail (end of K5 to end
of iteration) and the ratios.
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
    ap.add_argument("--holdout", type=float, default=0.10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10)
    # K5's bandwidth depends on where a session's tensor pool landed physically
    # (DESIGN.md §3): by default both sessions probe for a fast placement, as
    # bench.py's do; --no-probe keeps each session's first allocation, and
    # --holdout-first creates the holdout session before the masked one
    ap.add_argument("--no-probe", action="store_true")
    ap.add_argument("--holdout-first", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "holdout_admm", "holdout_admm_timing.json"))
    a = ap.parse_args()
    n, r = a.n, a.r
    d = synth.low_rank_plus_outliers(n, n, n, r)
    rng = np.random.default_rng(7)
    observed = np.asfortranarray(rng.random(d["D"].shape) >= a.missing)
    H = np.asfortranarray(observed & (rng.random(d["D"].shape) < a.holdout))
    opts = dict(synth.TRAFFIC_OPTS, tol=0.0, maxIter=a.warmup + 2 * a.rounds * a.iters + 1)
    kw = dict(n1=n, n2=n, n3=n, D=d["D"], device=0, probe=not a.no_probe)
    make = {"masked": lambda: tritd.Session(r, opts, d["A0"], d["B0"], d["C0"], observed=observed & ~H, **kw),
            "holdout": lambda: tritd.Session(r, opts, d["A0"], d["B0"], d["C0"], observed=observed,
                                             holdout=H, patience=0, **kw)}
    first = ("holdout", "masked") if a.holdout_first else ("masked", "holdout")
    made = {name: make[name]() for name in first}
    sess = {name: made[name] for name in ("masked", "holdout")}
    k5 = {k: [] for k in sess}
    it = {k: [] for k in sess}
    itev = {k: [] for k in sess}
    score, tail = [], []
    for s in sess.values():
        s.run(a.warmup)
        s.sync()
    for _ in range(a.rounds):
        for name, s in sess.items():
            s.set_timing(True)
            s.run(a.iters)
            s.sync()
            ms = s.kernel_ms()
            k5[name].append(ms["fused_update"])
            itev[name].append(ms["iteration"])
            if name == "holdout":
                sc, tl = s.holdout_ms()
                score.append(sc)
                tail.append(tl)
            s.set_timing(False)
            t0 = time.perf_counter()
            s.run(a.iters)
            s.sync()
            it[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
    held = int(sess["holdout"].holdout_info()[0])
    out = dict(shape=[n, n, n], r=r, missing=a.missing, holdout=a.holdout, iters=a.iters, rounds=a.rounds,
               probe=not a.no_probe, created_first=first[0], fitted=int(sess["holdout"].mask_info()[1]), held_out=held)

    def stat(key, xs):
        out[key] = round(statistics.median(xs), 5)
        out[key + "_min_max"] = [round(min(xs), 5), round(max(xs), 5)]

    for name in sess:
        stat("k5_ms_" + name, k5[name])
        stat("iter_ms_" + name, it[name])
        stat("iter_event_ms_" + name, itev[name])
        out["iters_done_" + name] = sess[name].sync()[0]
    stat("score_ms", score)
    stat("tail_ms", tail)
    # bytes the score kernel moves: T, the compact values, 32 B of words + 8 B of offset per tile
    nbytes = 8.0 * n * n * n + 8.0 * held + 40.0 * (n * n * n / 256)
    out["score_bytes"] = int(nbytes)
    out["score_TBps"] = round(nbytes / (out["score_ms"] * 1e-3) / 1e12, 4)
    res = {name: s.get() for name, s in sess.items()}
    out["errHist_equal"] = bool(np.array_equal(res["masked"]["errHist"], res["holdout"]["errHist"]))
    out["best_iter"] = res["holdout"]["best_iter"]
    for key in ("k5", "iter", "iter_event"):
        out[key + "_ratio"] = round(out[key + "_ms_holdout"] / out[key + "_ms_masked"], 5)
    for s in sess.values():
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
