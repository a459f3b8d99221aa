"""The goldens of the held-out validation of the masked nonconvex solver
(tests/golden/hnc*.npz) and what each is held to.  Shared by
tests/test_holdout_ncvx_oracle.py (CPU) and tests/test_gpu_holdout_ncvx.py (GPU).

Tolerances are those tests/masked_ncvx_cases.py uses for the onc* goldens, with
valHist and valHist1 at RTOL_ERR / ATOL_ERR like errHist.  Admission
(tests/golden/make_holdout_ncvx_golden.py): O is active, both scores are
finite, the stored drift of every compared quantity is at least MARGIN = 100x
below its tolerance, no perturbed run decides differently, and every comparison
that decides best_iter or a stop has a relative margin of at least
DECISION_MARGIN = 1e-6, 100x RTOL_ERR: a GPU result inside the tolerances
cannot flip one, so k, best_iter and stop_reason are compared exactly.
"""
import glob
import json
import os

import numpy as np

from conftest import GOLDEN, load_golden
from masked_ncvx_cases import ATOL_ERR, MARGIN, NCVX_KEYS, PARAM_KEYS, RTOL_ERR, TOL  # noqa: F401

DECISION_MARGIN = 1e-6
# drift name -> the tolerance it is held MARGIN below (gates are in units of the gate)
DRIFTS = dict(L=TOL, O=TOL, ABC=TOL, best_ABC=TOL, errHist_gate=1.0, valHist_gate=1.0,
              valHist1_gate=1.0)


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "hnc*.npz")))


def load(name):
    g = load_golden(name)
    if not isinstance(g["opts"], dict):
        g["opts"] = json.loads(str(g["opts"]))
    for key in ("observed", "holdout"):
        g[key] = np.asfortranarray(g[key].astype(bool))
    for key in ("r", "k", "patience", "val_norm", "best_iter", "best_iter_other", "stop_reason"):
        g[key] = int(g[key])
    g["fit"] = g["observed"] & ~g["holdout"]       # Omega & ~H
    g["held_out"] = g["observed"] & g["holdout"]   # H & Omega
    g["name"] = name
    return g


def padded_rank(r):
    return (r * r + 15) // 16 * 16


def args(g, **over):
    """The eight positional parameters of test.m:1 after (X, r), from a golden."""
    o = dict(g["opts"], **over)
    return [o[k] for k in PARAM_KEYS]


def ncvx_dict(prm):
    """args() -> the ncvx= dictionary of tritd.NcvxSession."""
    return dict(zip(NCVX_KEYS, prm[:6]))


def rel(a, b):
    den = np.linalg.norm(np.ravel(b))
    return float(np.linalg.norm(np.ravel(a - b)) / (den if den > 0 else 1.0))


def decision_margins(hist):
    """|hist(k) - running best| / running best for k >= 2: the comparisons that
    decide best_iter and the patience stop."""
    out, best = [], hist[0]
    for v in hist[1:]:
        out.append(abs(v - best) / best)
        best = min(best, v)
    return np.array(out)


def stop_margins(errHist, tol):
    """| |e(k) - e(k-1)| - tol e(k-1) | / (tol e(k-1)) for k >= 2: the test of
    :65 (tol = 0: |e(k) - e(k-1)| / e(k-1), the test fires on no change only)."""
    e = np.asarray(errHist)
    if tol == 0.0:
        return np.abs(e[1:] - e[:-1]) / e[:-1]
    rhs = tol * e[:-1]
    return np.abs(np.abs(e[1:] - e[:-1]) - rhs) / rhs


def rank_selection_case():
    """tests/holdout_als_cases.rank_selection_case (35 x 22 x 36, planted rank
    3, 1 % noise, 30 % missing, candidates (2, 3, 5), 15 % of the observed
    entries held out) for the nonconvex solver: the parameters of
    sweep_cases.NCVX_PARAMS at 40 iterations and gamma_A in (1e-3, 1e-2).
    lambda is no axis of the grid: the factor updates :49-51 read X, not Y, so
    lambda moves O and errHist and leaves both score histories bit for bit.
    The oracle's minimum valHist is 1.09e-2 at (3, 1e-3), 1.28e-2 at (5, 1e-3),
    6.8e-2 and more at gamma_A = 1e-2 and 0.63 at r = 2, while the last errHist
    is smallest at (2, 1e-3) (tests/test_holdout_ncvx_oracle.py)."""
    import holdout_als_cases as hac
    import sweep_cases as sc
    c = hac.rank_selection_case()
    names_ = ("rho", "lam", "gamma_A", "epsilon", "p", "theta", "maxIter", "tol")
    return dict(c, opts=dict(zip(names_, sc.ncvx_args(dict(maxIter=40)))), gammas=(1e-3, 1e-2))
