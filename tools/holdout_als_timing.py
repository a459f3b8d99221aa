#!/usr/bin/env python3
"""Cost of the held-out error in the ALS fit kernel: one holdout and one masked
AlsSession of the same fit on the same GPU, timed in alternating runs.

    python tools/holdout_als_timing.py [--n 512] [--r 8] [--missing 0.15] [--holdout 0.10]
                                       [--iters 20] [--rounds 6]
                                       [--out profiles/holdout_als/holdout_als_timing.json]

The problem is synth.low_rank_plus_outliers(n, n, n, r) in fp64 with tol = 0
and patience = 0 (nothing stops).  `missing` of the entries are unobserved and
`holdout` of the observed ones are held out; the masked session (the
yardstick: the fit kernel as it was before the holdout form existed) gets
observed = Omega & ~H, so both fit the same entries.  Each round runs `iters`
iterations on the masked session, then on the holdout one, first with the fit
kernel and the mode-3 contraction between events (set_timing) and then untimed
for the wall-clock iteration time.  Per tile the holdout form reads one 64 B
piece of mask words instead of 32 B and adds 8 v_readlane, 4 selects,
4 subtractions and 4 multiply-adds per lane; per iteration it adds the
one-thread finish's valHist bookkeeping and the snapshot kernel (a copy of
A, B, C when the iteration is the best so far, else an early exit).  Prints
one JSON line (and writes it to --out): the medians over the rounds of fit ms,
mode-3 ms and iteration ms for both, and their ratios.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "holdout_als", "holdout_als_timing.json"))
    a = ap.parse_args()
    n, r = a.n, a.r
    d = synth.low_rank_plus_outliers(n, n, n, r)
    rng = np.random.default_rng(7)
    observed = np.asfortranarray(rng.random(d["D"].shape) >= a.missing)
    H = np.asfortranarray(observed & (rng.random(d["D"].shape) < a.holdout))
    opts = dict(tol=0.0, maxIter=a.warmup + 2 * a.rounds * a.iters + 1)
    kw = dict(n1=n, n2=n, n3=n, X=d["D"], device=0, quiet=True)
    sess = {"masked": tritd.AlsSession(r, opts, d["A0"], d["B0"], d["C0"], observed=observed & ~H, **kw),
            "holdout": tritd.AlsSession(r, opts, d["A0"], d["B0"], d["C0"], observed=observed, holdout=H,
                                        patience=0, **kw)}
    fit = {k: [] for k in sess}
    m3 = {k: [] for k in sess}
    it = {k: [] for k in sess}
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
            s.set_timing(False)
            t0 = time.perf_counter()
            s.run(a.iters)
            s.sync()
            it[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = dict(shape=[n, n, n], r=r, missing=a.missing, holdout=a.holdout, iters=a.iters, rounds=a.rounds,
               fitted=int(sess["holdout"].mask_info()[1]), held_out=int(sess["holdout"].holdout_info()[0]))
    for name in sess:
        out["fit_ms_" + name] = round(statistics.median(fit[name]), 5)
        out["fit_ms_" + name + "_min_max"] = [round(min(fit[name]), 5), round(max(fit[name]), 5)]
        out["mode3_ms_" + name] = round(statistics.median(m3[name]), 5)
        out["iter_ms_" + name] = round(statistics.median(it[name]), 5)
        done, stopped = sess[name].sync()
        out["iters_done_" + name] = done
    res = {name: s.get() for name, s in sess.items()}
    out["errHist_equal"] = bool(np.array_equal(res["masked"]["errHist"], res["holdout"]["errHist"]))
    out["best_iter"] = res["holdout"]["best_iter"]
    for key in ("fit", "mode3", "iter"):
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
