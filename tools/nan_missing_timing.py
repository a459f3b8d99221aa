#!/usr/bin/env python3
"""What the mask preparation costs in front of a one-shot masked ADMM call, and
what observed="nan" saves of it.

    python tools/nan_missing_timing.py [--n 512] [--r 8] [--missing 0.15] [--iters 20]
                                       [--rounds 6] [--out FILE]

The input is synth.low_rank_plus_outliers(n, n, n, r) in fp64 with NaN at
`missing` of its entries, the traffic opts, maxIter = iters, tol = 0, one GPU.
Each round makes the same call to triple_decomp_ADMM in two ways, alternating:

  explicit  the path without observed="nan": observed = ~np.isnan(Dn) built
            inside the timed region, then the byte array of api._observed_bytes
            and its upload;
  nan       observed="nan": no host pass, no mask array.

Per way: the whole call (`total_ms`), the host time before the library is
entered (`host_ms`: the mask passes, the output allocations) and the library
call itself (`lib_ms`; the C entry point is wrapped by a timer).  The library
exposes no timing of its session creation, so that part is measured from
outside: the constructor of a Session (probe=False) made both ways in the same
rounds (`create_ms`, the host mask passes included for `explicit`).  One
session of each kind with a probed pool placement then runs `iters` timed
iterations per round, alternating (`iter_ms`, from kernel_ms): the iteration
itself must not move.  The two results of the first round are asserted equal,
bit for bit.  Prints one JSON line (medians, min-max beside them) and writes it
to --out.
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
from tritd import api, synth  # noqa: E402


class Timed:
    """A C entry point that records when it was entered and how long it ran."""

    def __init__(self, fn):
        self.fn, self.entered, self.ms = fn, 0.0, 0.0

    def __call__(self, *args):
        self.entered = time.perf_counter()
        try:
            return self.fn(*args)
        finally:
            self.ms = (time.perf_counter() - self.entered) * 1e3


def stat(xs):
    return round(statistics.median(xs), 3), [round(min(xs), 3), round(max(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--r", type=int, default=8)
    ap.add_argument("--missing", type=float, default=0.15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, r = a.n, a.r
    d = synth.low_rank_plus_outliers(n, n, n, r)
    Dn = np.array(d["D"], dtype=np.float64, order="F", copy=True)
    Dn[np.random.default_rng(7).random(Dn.shape) < a.missing] = np.nan
    f = (d["A0"], d["B0"], d["C0"])
    opts = dict(synth.TRAFFIC_OPTS, tol=0.0, maxIter=a.iters)
    entry = api.lib.tritd_admm_masked_f64 = Timed(api.lib.tritd_admm_masked_f64)

    def explicit_mask():
        return ~np.isnan(Dn)

    ways = {"explicit": explicit_mask, "nan": lambda: "nan"}
    t = {w: dict(total_ms=[], host_ms=[], lib_ms=[], create_ms=[]) for w in ways}
    first, sess = {}, {}
    kw = dict(n1=n, n2=n, n3=n, D=Dn, device=0, probe=False)
    for rnd in range(a.rounds + 1):  # round 0 warms the device and the allocator up
        for w, observed in ways.items():
            t0 = time.perf_counter()
            res = tritd.triple_decomp_ADMM(Dn, r, opts, *f, device=0, return_iters=True,
                                           observed=observed())
            t1 = time.perf_counter()
            if rnd == 0:
                first[w] = res
                continue
            t[w]["total_ms"].append((t1 - t0) * 1e3)
            t[w]["host_ms"].append((entry.entered - t0) * 1e3)
            t[w]["lib_ms"].append(entry.ms)
            del res
            if w in sess:
                sess.pop(w).close()
            t0 = time.perf_counter()
            sess[w] = tritd.Session(r, opts, *f, observed=observed(), **kw)
            t[w]["create_ms"].append((time.perf_counter() - t0) * 1e3)
    for x, y in zip(first["explicit"], first["nan"]):
        assert np.array_equal(x, y), "the two ways disagree"
    observed_count = int(sess["nan"].mask_info()[1])
    assert sess["explicit"].mask_info() == sess["nan"].mask_info()
    out = dict(shape=[n, n, n], r=r, missing=a.missing, iters=a.iters, rounds=a.rounds,
               observed=observed_count, equal=True)
    for s in sess.values():
        s.close()
    # the iteration: one session of each kind with a probed pool placement (so
    # that both stream from a fast one), timed in alternating rounds
    kw["probe"] = True
    o = dict(opts, maxIter=5 + a.rounds * a.iters + 1)
    sess = {w: tritd.Session(r, o, *f, observed=observed(), **kw) for w, observed in ways.items()}
    it = {w: [] for w in ways}
    for s in sess.values():
        s.run(5)
        s.sync()
    for _ in range(a.rounds):
        for w, s in sess.items():
            s.set_timing(True)
            s.run(a.iters)
            s.sync()
            it[w].append(s.kernel_ms()["iteration"])
            s.set_timing(0)
    for w, s in sess.items():
        out["iter_ms_" + w], out["iter_ms_" + w + "_min_max"] = stat(it[w])
        s.close()
    for w in ways:
        for key, xs in t[w].items():
            out[key + "_" + w], out[key + "_" + w + "_min_max"] = stat(xs)
    for key in ("total_ms", "host_ms", "lib_ms", "create_ms"):
        out[key.replace("_ms", "_ratio")] = round(out[key + "_nan"] / out[key + "_explicit"], 4)
    out["iter_ratio"] = round(out["iter_ms_nan"] / out["iter_ms_explicit"], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
