"""Dev helper: do A/B builds of libtritd.so give bitwise-identical solves?
usage: python tools/ab_same.py lib1.so,lib2.so [n] [r] [iters]
       python tools/ab_same.py lib1.so,lib2.so cases
Runs the same session (synthetic n^3, rank r; `cases`: each case of
tests/k5_step_bits_cases.py, 6 iterations) with each library and compares
errHist, A, B, C, O, E and the dense-tile counter with the first library's,
bitwise.  (The compact-E slots themselves cannot be read through the ABI: E is
what get() decodes from them and from the overflowed tiles, and the counter
says how many tiles overflowed.)"""
import ctypes as C
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "triple-tensor-decomposition-with-admm_amd"))
import numpy as np  # noqa: E402
import tritd  # noqa: E402
from tritd import _lib, api, synth  # noqa: E402
paths = sys.argv[1].split(",")
cases = len(sys.argv) > 2 and sys.argv[2] == "cases"
if cases:
    sys.argv[2:] = []
n = int(sys.argv[2]) if len(sys.argv) > 2 else 256
r = int(sys.argv[3]) if len(sys.argv) > 3 else 8
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 12
def load(p):
    l = C.CDLL(os.path.abspath(p))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(l, name):
            fn = getattr(l, name); fn.restype = res; fn.argtypes = args
    return l


def compare(label, run):
    """run() with each library in turn; everything against the first one's."""
    ref = None
    for p in paths:
        api.lib = _lib.lib = libs[p]
        out = run()
        if ref is None:
            ref = out
            print("%s %s: reference (k=%d, errHist[-1]=%.6e, dense tiles %s)"
                  % (label, p, out["k"], out["errHist"][-1], out["dense_tiles"]), flush=True)
            continue
        same = {k: bool(np.array_equal(np.asarray(out[k]), np.asarray(ref[k])))
                for k in ("errHist", "A", "B", "C", "O", "E", "dense_tiles")}
        print("%s %s: bitwise %s%s" % (label, p, same, "" if all(same.values()) else "  DIFFERENT"),
              flush=True)


def session_run(r, opts, d, n1, n2, n3, iters, observed=None):
    s = tritd.Session(r, opts, d["A0"], d["B0"], d["C0"], n1=n1, n2=n2, n3=n3, D=d["D"], device=0,
                      probe=False, observed=observed)
    s.run(iters); s.sync()
    out = s.get()
    out["dense_tiles"] = s.counters()
    s.close()
    return out


libs = {p: load(p) for p in paths}
if cases:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import k5_step_bits_cases as kc  # noqa: E402
    for cid in kc.IDS:
        c = kc.inputs(cid)
        os.environ.pop("TRITD_DENSE_E", None)
        if c["dense_e"]:
            os.environ["TRITD_DENSE_E"] = "1"
        compare(cid, lambda: session_run(c["r"], c["opts"], c, *c["D"].shape, kc.ITERS, c["observed"]))
    sys.exit(0)
n1 = n2 = n3 = n
if os.environ.get("AB_CFG", "4") == "5":  # 2048x2048x256 r=16 fp32 (bench.py --config 5)
    n1, n2, n3, r = 2048, 2048, 256, 16
    d = synth.low_rank_plus_outliers_f32(n1, n2, n3, r, p_out=0.05, seed=0, init_seed=123)
else:
    d = synth.low_rank_plus_outliers(n, n, n, r, p_out=0.05, seed=0, init_seed=123)
opts = dict(synth.TRAFFIC_OPTS, maxIter=iters)
compare("%dx%dx%d r=%d" % (n1, n2, n3, r), lambda: session_run(r, opts, d, n1, n2, n3, iters))
