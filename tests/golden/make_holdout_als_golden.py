"""Generate the golden vectors of the held-out validation error of the masked
ALS (tests/golden/hals*.npz).

The vectors come from tests/holdout_als_oracle.py.  Run from the repo root:

    python tests/golden/make_holdout_als_golden.py [name ...]

A golden reuses the inputs of a masked-ALS golden (`base`: X, observed, A0,
B0, C0, r of tests/golden/oals*.npz) and stores only the seeded H, patience,
opts (as JSON) and the outputs (A, B, C, errHist, k, valHist, best_iter,
stop_reason, A_best, B_best, C_best, holdout_count).

Admission rule (that of make_masked_als_golden.py): the oracle is rerun with
X, A0, B0 and C0 perturbed by 1e-15 relative (three seeds) and the worst drift
of every compared quantity is stored (drift_*); the perturbed reruns must take
the same k, best_iter and stop_reason.  H and patience of every case are chosen
so that each comparison of valHist(k) against the running best differs by at
least 1e-6 relative (tests/test_holdout_als_oracle.py asserts both).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "triple-tensor-decomposition-with-admm_amd"))

import holdout_als_oracle as hao  # noqa: E402
import masked_als_cases as mac  # noqa: E402
import tritd_oracle as orc  # noqa: E402

HOLD_SEED = 23
HOLD_FRACTION = 0.15
PERTURB = 1e-15
PERTURB_SEEDS = (1, 2, 3)

# name: (base golden, opts or None for the base's, patience)
CASES = {
    # padded rank 16; the stop test of :20 fires (stop_reason 1)
    "hals12x10x8_r2_stop": ("oals12x10x8_r2_stop", None, 0),
    # padded rank 32; a patience that never fires (stop_reason 0)
    "hals21x13x35_r5": ("oals21x13x35_r5", None, 2),
    # padded rank 48
    "hals18x19x22_r6": ("oals18x19x22_r6", None, 0),
    # padded rank 64: r^2 = 64 parameters per fibre overfit, valHist turns at
    # k = 4 and patience 3 stops the loop at k = 7 (stop_reason 2, 1 < best_iter < k)
    "hals17x16x20_r8_p3": ("oals17x16x20_r8", dict(maxIter=12, tol=0.0), 3),
    # five t-tiles: the odd tail of the walk
    "hals20x6x70_r3": ("oals20x6x70_r3", None, 0),
    # several ij-tiles (sharding), the three special tiles of the fit mask
    "hals30_r3_tiles": ("oals30_r3_tiles", None, 4),
    # every mode ragged
    "hals19x21x23_r7": ("oals19x21x23_r7", None, 0),
}


def case_inputs(name):
    base, opts, patience = CASES[name]
    g = mac.load(base)
    H = np.asfortranarray(np.random.default_rng(HOLD_SEED).random(g["X"].shape) < HOLD_FRACTION)
    return base, g, H, dict(g["opts"] if opts is None else opts), patience


def _rel(a, b):
    den = np.linalg.norm(np.ravel(b))
    return float(np.linalg.norm(np.ravel(a - b)) / (den if den > 0 else 1.0))


def _quiet(s):
    pass


def drifts(ref, g, H, opts, patience):
    A, B, C, eh, k, info = ref
    L = orc.triple_product(A, B, C)
    out = dict(L=0.0, ABC=0.0, errHist=0.0, valHist=0.0, k=0.0)
    for seed in PERTURB_SEEDS:
        rng = np.random.default_rng(seed)
        p = [np.asfortranarray(x * (1.0 + PERTURB * rng.standard_normal(x.shape)))
             for x in (g["X"], g["A0"], g["B0"], g["C0"])]
        A2, B2, C2, eh2, k2, i2 = hao.triple_decomp_ALS_holdout(p[0], g["observed"], H, g["r"], opts,
                                                                 p[1], p[2], p[3], patience, _quiet)
        same = (k2, i2["best_iter"], i2["stop_reason"]) == (k, info["best_iter"], info["stop_reason"])
        out["k"] = max(out["k"], 0.0 if same else 1.0)
        if not same:
            continue
        out["L"] = max(out["L"], _rel(orc.triple_product(A2, B2, C2), L))
        for x2, x in ((A2, A), (B2, B), (C2, C), (i2["A_best"], info["A_best"]),
                      (i2["B_best"], info["B_best"]), (i2["C_best"], info["C_best"])):
            out["ABC"] = max(out["ABC"], _rel(x2, x))
        out["errHist"] = max(out["errHist"], float(np.max(np.abs(eh2 - eh) / np.abs(eh))))
        out["valHist"] = max(out["valHist"], float(np.max(np.abs(i2["valHist"] - info["valHist"])
                                                           / np.abs(info["valHist"]))))
    return out


def make(name):
    base, g, H, opts, patience = case_inputs(name)
    ref = hao.triple_decomp_ALS_holdout(g["X"], g["observed"], H, g["r"], opts, g["A0"], g["B0"],
                                        g["C0"], patience, _quiet)
    A, B, C, eh, k, info = ref
    out = dict(base=np.array(base), holdout=H, patience=np.int64(patience), r=np.int64(g["r"]),
               opts=np.array(json.dumps(opts)), A=A, B=B, C=C, errHist=eh, k=np.int64(k),
               valHist=info["valHist"], best_iter=np.int64(info["best_iter"]),
               stop_reason=np.int64(info["stop_reason"]), A_best=info["A_best"],
               B_best=info["B_best"], C_best=info["C_best"],
               holdout_count=np.int64(info["holdout_count"]))
    dr = drifts(ref, g, H, opts, patience)
    for key, v in dr.items():
        out["drift_" + key] = np.float64(v)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    return k, info, dr


if __name__ == "__main__":
    for n in (sys.argv[1:] or CASES):
        k, info, dr = make(n)
        print(n, "k=%d best_iter=%d stop_reason=%d min valHist=%.3e" %
              (k, info["best_iter"], info["stop_reason"], info["valHist"].min()),
              " ".join("%s=%.1e" % kv for kv in dr.items()))
