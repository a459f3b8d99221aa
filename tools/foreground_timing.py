#!/usr/bin/env python3
"""What the detection mask and its score cost after a solve: the download of O
and a host threshold against Session.foreground.

    python tools/foreground_timing.py [--cases c3 c4] [--rounds 6] [--out FILE]

Cases: c3 = 240 x 320 x 300, r = 5 (synth.video_like) and c4 = 512^3, r = 8
(synth.low_rank_plus_outliers), fp64, 20 iterations.  Each case runs in a
child process of its own under `timeout`; the exit status of every child is
checked here and the first bad one ends the run.  In the child, on one
session, `rounds` alternating rounds time
  (a) get() of O (and everything else get() brings), np.abs(O) > thr and the
      oracle-style counts on the host: what a caller had to do before;
  (b) Session.foreground with a host ground truth and a host mask.
For (b) the kernel's own time comes from HIP events around its launch
(Session.foreground_ms), with the bytes it streams (D, Y_L, T, the labels, the
mask; mask words when the session has a mask) and the share of 8 TB/s that
makes.  The download of O alone, which (a) cannot avoid, is timed too
(tritd_session_get with O only).  Medians over the rounds; one JSON document
with a record per case goes to --out (default
profiles/foreground/foreground_timing.json) and to stdout.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "triple-tensor-decomposition-with-admm_amd")
CASES = {"c3": dict(shape=(240, 320, 300), r=5, kind="video", limit=420),
         "c4": dict(shape=(512, 512, 512), r=8, kind="lowrank", limit=540)}
THR = 50.0
HBM_PEAK = 8.0e12  # bytes/s


def host_counts(p, G):
    """eval's counts (video_triple_comparison.m:342-360) on the host, per frame"""
    import numpy as np
    g, m = G == 255, G == 170
    ax = (0, 1)
    return np.stack([(p & (g | m)).sum(axis=ax), (p & ~g).sum(axis=ax), (~p & g).sum(axis=ax),
                     (~p & (~g | m)).sum(axis=ax)], axis=1).astype(np.int64)


def child(name, rounds, iters):
    sys.path.insert(0, PKG)
    import numpy as np
    import tritd
    from tritd import _lib, synth
    c = CASES[name]
    n1, n2, n3 = c["shape"]
    d = synth.video_like(n1, n2, n3, c["r"]) if c["kind"] == "video" else \
        synth.low_rank_plus_outliers(n1, n2, n3, c["r"])
    opts = dict(synth.VIDEO_OPTS if c["kind"] == "video" else synth.TRAFFIC_OPTS, tol=0.0,
                maxIter=iters)
    G = np.asfortranarray(np.random.default_rng(3).choice(
        np.array([0, 50, 85, 170, 255], dtype=np.uint8), size=(n1, n2, n3), p=[.8, .04, .04, .04, .08]))
    s = tritd.Session(c["r"], opts, d["A0"], d["B0"], d["C0"], n1=n1, n2=n2, n3=n3, D=d["D"],
                      device=0, probe=False)
    s.run(iters)
    s.sync()
    s.set_timing(1)
    O = np.zeros((n1, n2, n3), order="F")
    t_a, t_b, t_o, t_k = [], [], [], []
    same = True
    for _ in range(rounds):
        t0 = time.perf_counter()
        got = s.get()
        pa = np.abs(got["O"]) > THR
        ca = host_counts(pa, G)
        t_a.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        fg = s.foreground(THR, G)
        t_b.append((time.perf_counter() - t0) * 1e3)
        t_k.append(s.foreground_ms())
        t0 = time.perf_counter()  # the download of O alone
        _lib.check(_lib.lib.tritd_session_get(s._s, None, None, None, C.c_void_p(O.ctypes.data), None,
                                              n1, None, None))
        t_o.append((time.perf_counter() - t0) * 1e3)
        same = same and bool((fg["mask"] == pa).all() and (fg["counts"] == ca).all())
    s.close()
    N = n1 * n2 * n3
    n1p, n3p = -(-n1 // 16) * 16, -(-n3 // 16) * 16
    streamed = 3 * 8 * (n1p * n2 * n3p) + 2 * N  # D, Y_L, T (padded) + labels + mask
    med = statistics.median
    k_ms = med(t_k)
    rec = dict(case=name, shape=[n1, n2, n3], r=c["r"], iters=iters, rounds=rounds, thr=THR,
               a_get_threshold_count_ms=round(med(t_a), 3), b_foreground_ms=round(med(t_b), 3),
               o_download_alone_ms=round(med(t_o), 3), kernel_ms=round(k_ms, 4),
               kernel_ms_min_max=[round(min(t_k), 4), round(max(t_k), 4)],
               bytes_streamed=streamed, kernel_GBps=round(streamed / k_ms / 1e6, 1),
               fraction_of_8TBps=round(streamed / (k_ms * 1e-3) / HBM_PEAK, 4),
               positives=int(fg["mask"].sum()), results_equal=same,
               b_cheaper_than_o_download=bool(med(t_b) < med(t_o)))
    print("FOREGROUND_TIMING " + json.dumps(rec), flush=True)
    return 0 if same else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["c3", "c4"], choices=list(CASES))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foreground",
                                                  "foreground_timing.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.exit(child(a.child, a.rounds, a.iters))
    records = []
    for name in a.cases:
        cmd = ["timeout", "-k", "10", str(CASES[name]["limit"]), sys.executable,
               os.path.abspath(__file__), "--child", name, "--rounds", str(a.rounds), "--iters",
               str(a.iters)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-4000:])
        if p.returncode != 0:
            sys.stdout.write(p.stdout[-4000:])
            print("foreground_timing: case %s ended with status %d; stopping" % (name, p.returncode))
            sys.exit(p.returncode)
        line = [x for x in p.stdout.splitlines() if x.startswith("FOREGROUND_TIMING ")][-1]
        records.append(json.loads(line.split(" ", 1)[1]))
    doc = dict(tool="tools/foreground_timing.py", cases=records)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
