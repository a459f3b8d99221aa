"""Generate the golden vectors of the held-out validation of the masked
nonconvex solver (tests/golden/hnc*.npz).

The vectors come from tests/holdout_ncvx_oracle.py.  Run from the repo root:

    python tests/golden/make_holdout_ncvx_golden.py [--dry] [name ...]

Each .npz holds the inputs (X, observed, holdout, A0, B0, C0, r, the eight
parameters of test.m:1 as JSON in `opts`, patience, val_norm) and the outputs
(A, B, C, O, errHist, k, valHist, valHist1, best_iter, stop_reason, A_best,
B_best, C_best), plus best_iter_other: the best iterate the other val_norm
would have chosen on the same run.

The parameters are those of the nc*.npz goldens (tests/golden/make_golden.py),
the data tritd.synth.low_rank_plus_outliers.

Admission (asserted here and again by tests/test_holdout_ncvx_oracle.py):
* O is active: nonzero at some fitted entries, but not at all of them;
* both score histories are finite;
* every comparison that decides best_iter or a stop (the chosen history against
  its running best; |errHist(k) - errHist(k-1)| against tol errHist(k-1)) has a
  relative margin of at least 1e-6;
* the drift rule of make_masked_ncvx_golden.py: the oracle rerun with X, A0, B0,
  C0 perturbed by 1e-15 relative (three seeds) moves every compared quantity,
  both score histories included, by at least 100x less than its tolerance, and
  moves no decision.
A case that fails gets another seed or a shorter maxIter, never a looser rule.
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

import holdout_ncvx_oracle as hno  # noqa: E402
import tritd_oracle as orc  # noqa: E402
from tritd import drivers, synth  # noqa: E402

TOL, RTOL_ERR, ATOL_ERR, MARGIN = 1e-9, 1e-8, 1e-13, 100.0  # tests/masked_ncvx_cases.py
DECISION_MARGIN = 1e-6
PERTURB = 1e-15
PERTURB_SEEDS = (1, 2, 3)
PARAM_KEYS = ("rho", "lambda", "gamma_A", "epsilon", "p", "theta", "maxIter", "tol")
NCVX_PARAMS = dict(rho=1.0, **{"lambda": 0.5}, gamma_A=1e-3, epsilon=1e-2, p=0.5, theta=2.0 / 3.0)

# name: dict(shape, r, seed, missing, ratio, maxIter, patience, val_norm, tol, blocks)
CASES = {
    # RP = 16, one ragged tile; the loop stops by patience with 1 < best_iter < k
    "hnc12x10x8_r2_p": dict(shape=(12, 10, 8), r=2, seed=2, missing=0.20, ratio=0.15, maxIter=30,
                            patience=2, val_norm=2),
    # RP = 16, several tiles, a tile held out whole, a tile with none, flags outside Omega
    "hnc30_r3_tiles": dict(shape=(30, 30, 30), r=3, seed=3, missing=0.15, ratio=0.10, maxIter=10,
                           patience=0, val_norm=2, blocks=True),
    # RP = 16, five t-tiles; val_norm = 1
    "hnc20x6x70_r3_l1": dict(shape=(20, 6, 70), r=3, seed=3, missing=0.15, ratio=0.10, maxIter=10,
                             patience=0, val_norm=1),
    # RP = 32
    "hnc21x13x35_r5": dict(shape=(21, 13, 35), r=5, seed=5, missing=0.10, ratio=0.10, maxIter=10,
                           patience=0, val_norm=2),
    # RP = 48
    "hnc18x19x22_r6": dict(shape=(18, 19, 22), r=6, seed=6, missing=0.10, ratio=0.10, maxIter=10,
                           patience=0, val_norm=2),
    # RP = 64, a 1-row edge tile; the test of :65 fires before maxIter
    "hnc17x16x20_r8_stop": dict(shape=(17, 16, 20), r=8, seed=8, missing=0.10, ratio=0.10,
                                maxIter=12, patience=0, val_norm=2, tol=0.1),
}


def case_inputs(name):
    c = CASES[name]
    n1, n2, n3 = c["shape"]
    d = synth.low_rank_plus_outliers(n1, n2, n3, c["r"], seed=c["seed"], init_seed=c["seed"] + 100)
    observed = np.asfortranarray(np.random.default_rng([c["seed"], 7]).random(d["D"].shape) >= c["missing"])
    if c.get("blocks"):
        observed[:16, 0, :16] = True
    H = drivers.holdout_mask(observed, c["ratio"], np.random.default_rng([c["seed"], 11]))
    if c.get("blocks"):
        H[:16, 0, :16] = True    # a 16 x 16 (i, t) tile held out whole
        H[:16, 1, :16] = False   # a tile without a held-out element
        H[16:, 2, 16:] = True    # flags outside Omega as well: they are ignored
    prm = dict(NCVX_PARAMS, maxIter=c["maxIter"], tol=c.get("tol", 0.0))
    return (dict(X=d["D"], A0=d["A0"], B0=d["B0"], C0=d["C0"]), observed, np.asfortranarray(H), c["r"],
            prm, c["patience"], c["val_norm"])


def args(prm):
    return [prm[k] for k in PARAM_KEYS]


def decision_margins(hist):
    """|hist(k) - running best| / running best for k >= 2."""
    out, best = [], hist[0]
    for v in hist[1:]:
        out.append(abs(v - best) / best)
        best = min(best, v)
    return np.array(out)


def stop_margins(errHist, tol):
    """| |e(k) - e(k-1)| - tol e(k-1) | / (tol e(k-1)) for k >= 2 (:65); with
    tol = 0 the test cannot fire unless errHist repeats: |e(k) - e(k-1)| / e(k-1)."""
    e = np.asarray(errHist)
    if tol == 0.0:
        return np.abs(e[1:] - e[:-1]) / e[:-1]
    rhs = tol * e[:-1]
    return np.abs(np.abs(e[1:] - e[:-1]) - rhs) / rhs


def first_argmin(hist):
    best, at = hist[0], 1
    for k, v in enumerate(hist[1:], start=2):
        if v < best:
            best, at = v, k
    return at


def _rel(a, b):
    den = np.linalg.norm(np.ravel(b))
    return float(np.linalg.norm(np.ravel(a - b)) / (den if den > 0 else 1.0))


def _gate(a, b):
    return float(np.max(np.abs(a - b) / (RTOL_ERR * np.abs(b) + ATOL_ERR)))


def drifts(ref, d, observed, H, r, prm, patience, val_norm):
    L = orc.triple_product(ref["A"], ref["B"], ref["C"])
    out = dict(L=0.0, O=0.0, ABC=0.0, best_ABC=0.0, errHist_gate=0.0, valHist_gate=0.0,
               valHist1_gate=0.0, decisions=0.0)
    for seed in PERTURB_SEEDS:
        rng = np.random.default_rng(seed)
        p = [np.asfortranarray(x * (1.0 + PERTURB * rng.standard_normal(x.shape)))
             for x in (d["X"], d["A0"], d["B0"], d["C0"])]
        q = hno.triple_decomp_ncvx_holdout(p[0], observed, H, r, *args(prm), p[1], p[2], p[3],
                                           patience, val_norm)
        same = all(q[key] == ref[key] for key in ("k", "best_iter", "stop_reason"))
        out["decisions"] = max(out["decisions"], 0.0 if same else 1.0)
        if not same:
            continue
        out["L"] = max(out["L"], _rel(orc.triple_product(q["A"], q["B"], q["C"]), L))
        out["O"] = max(out["O"], _rel(q["O"], ref["O"]))
        for key in "ABC":
            out["ABC"] = max(out["ABC"], _rel(q[key], ref[key]))
            out["best_ABC"] = max(out["best_ABC"], _rel(q[key + "_best"], ref[key + "_best"]))
        for key in ("errHist", "valHist", "valHist1"):
            out[key + "_gate"] = max(out[key + "_gate"], _gate(q[key], ref[key]))
    return out


def admitted(g):
    """The admission conditions on a golden (a dict as stored); a list of the
    failures, empty when it passes."""
    bad = []
    fit = g["observed"].astype(bool) & ~g["holdout"].astype(bool)
    nz = np.count_nonzero(np.asarray(g["O"])[fit])
    if not 0 < nz < np.count_nonzero(fit):
        bad.append("O is not active: %d of %d fitted entries" % (nz, np.count_nonzero(fit)))
    if np.asarray(g["O"])[~fit].any():
        bad.append("O is nonzero outside the fit mask")
    if not (np.all(np.isfinite(g["valHist"])) and np.all(np.isfinite(g["valHist1"]))):
        bad.append("a score is not finite")
    for key, tol in (("L", TOL), ("O", TOL), ("ABC", TOL), ("best_ABC", TOL), ("errHist_gate", 1.0),
                     ("valHist_gate", 1.0), ("valHist1_gate", 1.0)):
        if not float(g["drift_" + key]) * MARGIN <= tol:
            bad.append("drift_%s = %.2e" % (key, float(g["drift_" + key])))
    if float(g["drift_decisions"]) != 0.0:
        bad.append("a perturbed run decided differently")
    hist = g["valHist1"] if int(g["val_norm"]) == 1 else g["valHist"]
    dm = decision_margins(np.asarray(hist))
    if dm.size and dm.min() < DECISION_MARGIN:
        bad.append("best_iter margin %.2e" % dm.min())
    opts = g["opts"] if isinstance(g["opts"], dict) else json.loads(str(g["opts"]))
    sm = stop_margins(g["errHist"], float(opts["tol"]))
    if sm.size and sm.min() < DECISION_MARGIN:
        bad.append("stop-test margin %.2e" % sm.min())
    return bad


def make(name):
    d, observed, H, r, prm, patience, val_norm = case_inputs(name)
    ref = hno.triple_decomp_ncvx_holdout(d["X"], observed, H, r, *args(prm), d["A0"], d["B0"],
                                         d["C0"], patience, val_norm)
    other = first_argmin(ref["valHist"] if val_norm == 1 else ref["valHist1"])
    out = dict(X=d["X"], observed=observed, holdout=H, A0=d["A0"], B0=d["B0"], C0=d["C0"],
               r=np.int64(r), opts=np.array(json.dumps(prm)), patience=np.int64(patience),
               val_norm=np.int64(val_norm), best_iter_other=np.int64(other))
    for key in ("A", "B", "C", "O", "errHist", "valHist", "valHist1", "A_best", "B_best", "C_best"):
        out[key] = ref[key]
    for key in ("k", "best_iter", "stop_reason"):
        out[key] = np.int64(ref[key])
    dr = drifts(ref, d, observed, H, r, prm, patience, val_norm)
    for key, v in dr.items():
        out["drift_" + key] = np.float64(v)
    bad = admitted(out)
    print(name, "k=%d best=%d (other %d) stop=%d" % (ref["k"], ref["best_iter"], other, ref["stop_reason"]),
          " ".join("%s=%.1e" % kv for kv in dr.items()), "REFUSED: " + "; ".join(bad) if bad else "ok")
    if "--verbose" in sys.argv:
        print("  valHist ", np.array2string(ref["valHist"], precision=4))
        print("  valHist1", np.array2string(ref["valHist1"], precision=4))
        print("  errHist ", np.array2string(ref["errHist"], precision=4))
    if not bad and "--dry" not in sys.argv:
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    return ref, bad


if __name__ == "__main__":
    for n in ([a for a in sys.argv[1:] if not a.startswith("--")] or CASES):
        make(n)
