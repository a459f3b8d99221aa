"""The goldens of the held-out validation error of the masked ALS
(tests/golden/hals*.npz) and what each is held to.  Shared by
tests/test_holdout_als_oracle.py (CPU) and tests/test_gpu_holdout_als.py (GPU).

A golden reuses the inputs of the masked-ALS golden named in its `base`
(X, observed, A0, B0, C0, r; tests/golden/oals*.npz) and stores only the
seeded H, `patience`, its opts, the expected outputs and their drifts
(tests/golden/make_holdout_als_golden.py).

Tolerances are those of tests/masked_als_cases.py, with valHist at TOL_ERR /
ATOL_ERR like errHist.  The held rule is that module's: a golden is held to a
tolerance only where its stored drift (the oracle rerun with inputs perturbed
by 1e-15 relative) is at least 100x below it.  k, best_iter and stop_reason
are compared exactly: every comparison that decides them (valHist(k) against
the running best) differs by at least DECISION_MARGIN relative, 1000x TOL_ERR,
so a GPU result inside the tolerance cannot flip one.
"""
import glob
import os

import numpy as np

import masked_als_cases as mac
from conftest import GOLDEN, load_golden

TOL_ABC, TOL_L, TOL_ERR, ATOL_ERR, MARGIN = mac.TOL_ABC, mac.TOL_L, mac.TOL_ERR, mac.ATOL_ERR, mac.MARGIN
DECISION_MARGIN = 1e-6

QUANTITIES = dict(mac.QUANTITIES, valHist=("drift_valHist", TOL_ERR))
DEFAULT = ("L", "ABC", "errHist", "valHist")
# goldens held for less than DEFAULT (see masked_als_cases.SPECIAL)
SPECIAL = {}


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "hals*.npz")))


def load(name):
    """The golden with the inputs of its base merged in."""
    g = load_golden(name)
    base = mac.load(str(g["base"]))
    for key in ("X", "observed", "A0", "B0", "C0"):
        g[key] = base[key]
    assert g["r"] == base["r"]
    g["holdout"] = g["holdout"].astype(bool)
    g["patience"] = int(g["patience"])
    g["best_iter"] = int(g["best_iter"])
    g["stop_reason"] = int(g["stop_reason"])
    g["fit"] = g["observed"] & ~g["holdout"]   # Omega & ~H
    g["held_out"] = g["observed"] & g["holdout"]  # H & Omega
    return g


def held(name):
    return SPECIAL.get(name, DEFAULT)


padded_rank = mac.padded_rank


def decision_margins(valHist):
    """|valHist(k) - running best| / running best for k >= 2: the comparisons
    that decide best_iter and the patience stop."""
    out, best = [], valHist[0]
    for v in valHist[1:]:
        out.append(abs(v - best) / best)
        best = min(best, v)
    return np.array(out)


def rank_selection_case():
    """masked_als_cases.completion_case (35 x 22 x 36, planted rank 3, 1 %
    noise, 30 % missing, 40 iterations), candidates (2, 3, 5), 15 % of the
    observed entries held out; the initial factors of rank r are drawn from a
    generator seeded by r."""
    d, observed, r, opts = mac.completion_case()
    n1, n2, n3 = d["X"].shape

    def factors(rr):
        rng = np.random.default_rng(4000 + rr)
        return (np.asfortranarray(rng.standard_normal((n1, rr, rr))),
                np.asfortranarray(rng.standard_normal((rr, n2, rr))),
                np.asfortranarray(rng.standard_normal((rr, rr, n3))))

    return dict(X=d["X"], observed=observed, ranks=(2, 3, 5), holdout_ratio=0.15, opts=opts, seed=7,
                planted=r, factors=factors)
