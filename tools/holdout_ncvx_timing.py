#!/usr/bin/env python3
"""Cost of the held-out scores of the masked nonconvex solver: one holdout
session (NcvxSession) and one masked nonconvex AlsSession of the same fit on
the same GPU, timed in alternating runs.

    python tools/holdout_ncvx_timing.py [--n 512] [--r 8] [--missing 0.15] [--holdout 0.10]
                                        [--iters 20] [--rounds 6] [--holdout-first]
                                        [--out profiles/holdout_ncvx/holdout_ncvx_timing.json]

The problem is synth.low_rank_plus_outliers(n, n, n, r) in fp64 with the
parameters of the nc*.npz goldens, tol = 0 and patience = 0 (nothing stops).
`missing` of the entries are unobserved and `holdout` of the observed ones are
held out; the masked session (the yardstick: the code path as it was before
this holdout existed) gets observed = Omega & ~H, so both fit the same entries
with the same fit kernel.  Each round runs `iters` iterations on the masked
session, then on the holdout one, first with events around the fit, the mode-3
contraction, the iteration and (holdout) the score kernel (set_timing) and then
untimed for the wall-clock iteration time.  Between its fit and its A update a
holdout iteration adds the score kernel (it reads the TX copy the fit wrote,
N x 8 B, the compact held-out values and 32 B of words and 8 B of offset per
tile), its pair reduction, the one-thread mark and the snapshot kernel.

An ALS session has no placement probe (the ADMM session's),
so each session keeps its first allocation; --holdout-first creates the holdout
session before the masked one, to tell the score's cost from the placement's.
Prints one JSON line (and writes it to --out): medians over the rounds with
min-max of fit, mode-3 and iteration ms for both, the score kernel's ms and
achieved bandwidth, the tail (end of the fit to the start of the A update), the
ratios, the untimed iteration ms of every round and the per-round difference
holdout - masked, and whether the two errHist arrays are bitwise equal.
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
    ap.add_argument("--holdout-first", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "holdout_ncvx", "holdout_ncvx_timing.json"))
    a = ap.parse_args()
    n, r = a.n, a.r
    d = synth.low_rank_plus_outliers(n, n, n, r)
    rng = np.random.default_rng(7)
    observed = np.asfortranarray(rng.random(d["D"].shape) >= a.missing)
    H = np.asfortranarray(observed & (rng.random(d["D"].shape) < a.holdout))
    opts = dict(tol=0.0, maxIter=a.warmup + 2 * a.rounds * a.iters + 1)
    ncvx = dict(rho=1.0, lam=0.5, gamma_A=1e-3, epsilon=1e-2, p=0.5, theta=2.0 / 3.0)
    kw = dict(n1=n, n2=n, n3=n, X=d["D"], device=0, quiet=True, ncvx=ncvx)
    make = {"masked": lambda: tritd.AlsSession(r, opts, d["A0"], d["B0"], d["C0"], observed=observed & ~H, **kw),
            "holdout": lambda: tritd.NcvxSession(r, opts, d["A0"], d["B0"], d["C0"], observed=observed,
                                                 holdout=H, patience=0, **kw)}
    first = ("holdout", "masked") if a.holdout_first else ("masked", "holdout")
    made = {name: make[name]() for name in first}
    sess = {name: made[name] for name in ("masked", "holdout")}
    fit = {k: [] for k in sess}
    m3 = {k: [] for k in sess}
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
            fit[name].append(ms["fit"])
            m3[name].append(ms["mode3"])
            itev[name].append(ms["iteration"])
            if name == "holdout":
                h = s.holdout_ms()
                score.append(h["score"])
                tail.append(h["tail"])
            s.set_timing(False)
            t0 = time.perf_counter()
            s.run(a.iters)
            s.sync()
            it[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
    held = int(sess["holdout"].holdout_info()[0])
    out = dict(solver="ncvx", shape=[n, n, n], r=r, missing=a.missing, holdout=a.holdout, iters=a.iters,
               rounds=a.rounds, created_first=first[0], fitted=int(sess["holdout"].mask_info()[1]),
               held_out=held)

    def stat(key, xs):
        out[key] = round(statistics.median(xs), 5)
        out[key + "_min_max"] = [round(min(xs), 5), round(max(xs), 5)]

    for name in sess:
        stat("fit_ms_" + name, fit[name])
        stat("mode3_ms_" + name, m3[name])
        stat("iter_ms_" + name, it[name])
        stat("iter_event_ms_" + name, itev[name])
        out["iters_done_" + name] = sess[name].sync()[0]
    # per round, in order: an iteration's cost can drift over a long run (the
    # pinv fallback of an ill-conditioned Gram), alike in both sessions
    for name in sess:
        out["iter_ms_rounds_" + name] = [round(x, 5) for x in it[name]]
    stat("iter_delta_ms", [h - m for h, m in zip(it["holdout"], it["masked"])])
    stat("score_ms", score)
    stat("tail_ms", tail)
    # bytes the score kernel moves: the TX copy, the compact values, 32 B of words + 8 B of offset per tile
    nbytes = 8.0 * n * n * n + 8.0 * held + 40.0 * (n * n * n / 256)
    out["score_bytes"] = int(nbytes)
    out["score_TBps"] = round(nbytes / (out["score_ms"] * 1e-3) / 1e12, 4)
    res = {name: s.get() for name, s in sess.items()}
    out["errHist_equal"] = bool(np.array_equal(res["masked"]["errHist"], res["holdout"]["errHist"]))
    out["best_iter"] = res["holdout"]["best_iter"]
    for key in ("fit", "mode3", "iter", "iter_event"):
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
