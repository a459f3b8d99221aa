#!/usr/bin/env python3
"""What the video driver's eight figures cost after a solve: the host path of
drivers.video_triple against Session.report.

    python tools/report_timing.py [--cases c3 c4] [--rounds 4] [--out FILE]

Cases: c3 = 240 x 320 x 300, r = 5 (synth.video_like) and c4 = 512^3, r = 8
(synth.low_rank_plus_outliers), fp64; the original tensor X is the case's D,
15 % of it missing (drivers.missing_mask) and zero-filled, 20 iterations.  Each
case runs in a child process of its own under `timeout`; the exit status of
every child is checked here and the first bad one ends the run.  In the child,
on one session, `rounds` alternating rounds time
  (a) what a caller does today (video_triple_comparison.m:56,64-67 as
      drivers.video_triple runs them): get(), triple_product, X_hat + O, three
      evaluate calls and quality_ybz;
  (b) Session.report with a host X and a host mask;
  (c) the same with X and the mask in device memory (TRITD_REPORT_DEVICE);
  (d) the kernels alone, from HIP events (tritd_session_report_ms), with and
      without SSIM.
For (d) without SSIM the record holds the bytes the pass streams (X, the mask
bytes, and D, Y_L, T in their padded tile-major size) with their share of
8 TB/s, and 2 N RP flops against the 78.6 TF/s f64 MFMA peak.  Every round
asserts that (a) and (b) agree within the tolerances of
tests/test_gpu_report.py, computed from (a)'s own tensors.  Medians over the
rounds; one JSON document with a record per case goes to --out (default
profiles/session_report/report_timing.json) and to stdout.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "triple-tensor-decomposition-with-admm_amd")
CASES = {"c3": dict(shape=(240, 320, 300), r=5, kind="video", limit=420),
         "c4": dict(shape=(512, 512, 512), r=8, kind="lowrank", limit=840)}
HBM_PEAK = 8.0e12   # bytes/s
F64_MFMA = 78.6e12  # flop/s (tools/bench_prims.py)
RTOL_SUM, TOL_TP = 1e-12, 1e-13          # tests/boundary_cases.py
SSIM_RTOL = 1e-11 + 10 * 1.11e-13        # tests/test_gpu_report.py
FIGURES = ("rmse", "nrmse", "srmse", "snrmse", "trmse", "tnrmse", "psnr", "ssim")


def host_path(tritd, s, X, mask, gt, gt_2):
    """drivers.video_triple after the solve -> (figures, X_hat, O)"""
    import numpy as np
    g = s.get()
    X_hat = tritd.triple_product(g["A"], g["B"], g["C"])
    rmse, nrmse = tritd.evaluate(X_hat, gt, mask)
    rmse2, nrmse2 = tritd.evaluate(g["O"], gt_2, ~mask)
    rmse3, nrmse3 = tritd.evaluate(np.asfortranarray(X_hat + g["O"]), X)
    psnr, ssim = tritd.quality_ybz(X, X_hat)
    return dict(zip(FIGURES, (rmse, nrmse, rmse2, nrmse2, rmse3, nrmse3, psnr, ssim))), X_hat, g["O"]


def figure_tolerances(X, mask, L, O):
    """relative tolerances of the eight figures, from (a)'s tensors alone"""
    import numpy as np
    nrm = lambda v: float(np.sqrt(np.dot(v.ravel(order="K"), v.ravel(order="K"))))
    moved = lambda P, D: RTOL_SUM + 2.0 * TOL_TP * nrm(P) / nrm(D)
    t0 = moved(L[mask], (L - X)[mask])
    P = L + O
    t4 = moved(P, P - X)
    tf = max(moved(L[:, :, f], L[:, :, f] - X[:, :, f]) for f in range(X.shape[2]))
    # a figure is a root, or a ratio of two roots, of sums within these
    return dict(rmse=t0, nrmse=t0 + RTOL_SUM, srmse=RTOL_SUM, snrmse=2 * RTOL_SUM, trmse=t4,
                tnrmse=t4 + RTOL_SUM, psnr_abs=10.0 / math.log(10.0) * tf, ssim=SSIM_RTOL)


def child(name, rounds, iters):
    sys.path.insert(0, PKG)
    import numpy as np
    import tritd
    from tritd import drivers, hip, synth
    c = CASES[name]
    n1, n2, n3 = c["shape"]
    d = synth.video_like(n1, n2, n3, c["r"]) if c["kind"] == "video" else \
        synth.low_rank_plus_outliers(n1, n2, n3, c["r"])
    opts = dict(synth.VIDEO_OPTS if c["kind"] == "video" else synth.TRAFFIC_OPTS, tol=0.0,
                maxIter=iters)
    X = np.asfortranarray(d["D"], dtype=np.float64)
    mask = drivers.missing_mask(X.shape, 0.15, np.random.default_rng(0))
    mask = np.asfortranarray(mask)
    Y = np.array(X, order="F", copy=True)
    Y[mask] = 0.0
    gt = X.ravel(order="F")[mask.ravel(order="F")]
    gt_2 = X.ravel(order="F")[~mask.ravel(order="F")]
    s = tritd.Session(c["r"], opts, d["A0"], d["B0"], d["C0"], n1=n1, n2=n2, n3=n3, D=Y, device=0,
                      probe=False)
    s.run(iters)
    s.sync()
    s.set_timing(1)
    dX, dM = hip.DeviceArray.from_host(X), hip.DeviceArray.from_host(mask.view(np.uint8))
    t_a, t_b, t_c, t_k, t_ks = [], [], [], [], []
    worst = dict.fromkeys(FIGURES, 0.0)
    tol, ok, same_bits = None, True, True
    try:
        for _ in range(rounds):
            t0 = time.perf_counter()
            fa, X_hat, O = host_path(tritd, s, X, mask, gt, gt_2)
            t_a.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            fb = s.report(X, mask)
            t_b.append((time.perf_counter() - t0) * 1e3)
            t_ks.append(s.report_ms())
            t0 = time.perf_counter()
            fc = s.report(x_device_ptr=dX.ptr, missing_device_ptr=dM.ptr)
            t_c.append((time.perf_counter() - t0) * 1e3)
            s.report(x_device_ptr=dX.ptr, missing_device_ptr=dM.ptr, ssim=False)
            t_k.append(s.report_ms())
            if tol is None:
                tol = figure_tolerances(X, mask, X_hat, O)
            del X_hat, O
            for k in FIGURES:
                if k == "psnr":
                    good = abs(fb[k] - fa[k]) <= tol["psnr_abs"] + 1e-13 * abs(fa[k])
                    worst[k] = max(worst[k], abs(fb[k] - fa[k]))
                else:
                    rel = abs(fb[k] - fa[k]) / abs(fa[k])
                    good = rel <= tol[k]
                    worst[k] = max(worst[k], rel)
                if not good:
                    ok = False
                    print("report_timing: %s differs: host %r session %r" % (k, fa[k], fb[k]), flush=True)
            same_bits = same_bits and all(fb[k] == fc[k] for k in FIGURES)
    finally:
        dX.free()
        dM.free()
        s.close()
    N = n1 * n2 * n3
    RP = -(-(c["r"] ** 2) // 16) * 16
    n1p, n3p = -(-n1 // 16) * 16, -(-n3 // 16) * 16
    streamed = 8 * N + N + 3 * 8 * (n1p * n2 * n3p)  # X, the mask bytes, D, Y_L, T (padded)
    flops = 2 * N * RP
    med = statistics.median
    k_ms = med(t_k)
    rec = dict(case=name, shape=[n1, n2, n3], r=c["r"], RP=RP, iters=iters, rounds=rounds,
               a_host_path_ms=round(med(t_a), 3), b_report_host_ms=round(med(t_b), 3),
               c_report_device_ms=round(med(t_c), 3), d_kernels_ms=round(k_ms, 4),
               d_kernels_ms_min_max=[round(min(t_k), 4), round(max(t_k), 4)],
               d_kernels_with_ssim_ms=round(med(t_ks), 4),
               bytes_streamed=streamed, kernel_GBps=round(streamed / k_ms / 1e6, 1),
               fraction_of_8TBps=round(streamed / (k_ms * 1e-3) / HBM_PEAK, 4),
               flops=flops, fraction_of_f64_mfma_peak=round(flops / (k_ms * 1e-3) / F64_MFMA, 4),
               figures={k: fb[k] for k in FIGURES},
               tolerances=tol, worst_difference=worst, a_and_b_agree=ok,
               host_and_device_forms_same_bits=same_bits)
    print("REPORT_TIMING " + json.dumps(rec), flush=True)
    return 0 if ok and same_bits else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["c3", "c4"], choices=list(CASES))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_report",
                                                  "report_timing.json"))
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
            print("report_timing: case %s ended with status %d; stopping" % (name, p.returncode))
            sys.exit(p.returncode)
        line = [x for x in p.stdout.splitlines() if x.startswith("REPORT_TIMING ")][-1]
        records.append(json.loads(line.split(" ", 1)[1]))
    doc = dict(tool="tools/report_timing.py", cases=records)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
