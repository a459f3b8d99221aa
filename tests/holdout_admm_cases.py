"""The goldens of the held-out validation of the masked ADMM
(tests/golden/hadm*.npz) and what each is held to.  Shared by
tests/test_holdout_admm_oracle.py (CPU) and tests/test_gpu_holdout_admm.py (GPU).

Tolerances are those of tests/masked_cases.py, with valHist and valHist1 at
TOL_ERR / ATOL_ERR like errHist.  Admission (tests/golden/
make_holdout_admm_golden.py): the stored drift of every compared quantity (the
oracle rerun with inputs perturbed by 1e-15 relative) is at least MARGIN = 100x
below its tolerance, no perturbed run decides differently, and every comparison
that decides best_iter or a stop has a relative margin of at least
DECISION_MARGIN = 1e-6, 100x TOL_ERR: a GPU result inside the tolerances cannot
flip one, so k, best_iter and stop_reason are compared exactly.
"""
import glob
import json
import os

import numpy as np

from conftest import GOLDEN, load_golden
from masked_cases import ATOL_ERR, MARGIN, TOL_ABC, TOL_ERR, TOL_LOE  # noqa: F401

DECISION_MARGIN = 1e-6
# drift name -> the tolerance it is held MARGIN below (gates are in units of the gate)
DRIFTS = dict(L=TOL_LOE, O=TOL_LOE, E=TOL_LOE, ABC=TOL_ABC, best_ABC=TOL_ABC, errHist_gate=1.0,
              valHist_gate=1.0, valHist1_gate=1.0)


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "hadm*.npz")))


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


def decision_margins(hist):
    """|hist(k) - running best| / running best for k >= 2: the comparisons that
    decide best_iter and the patience stop."""
    out, best = [], hist[0]
    for v in hist[1:]:
        out.append(abs(v - best) / best)
        best = min(best, v)
    return np.array(out)


def stop_margins(errHist, tol):
    """| |e(k) - e(k-1)| - tol e(k-1) | / (tol e(k-1)) for k >= 2: the test of :63."""
    e = np.asarray(errHist)
    rhs = tol * e[:-1]
    return np.abs(np.abs(e[1:] - e[:-1]) - rhs) / rhs


def sweep_holdout(case):
    """H for tests/masked_sweep_cases.inputs(case): 10 % of the observed entries
    (default_rng([r, 13])), the fully observed tile [:16, 3, :16] held out
    whole, no held-out element in [:16, 4, :16], and flags on the wholly
    missing tile [:16, 1, 16:32] (outside Omega: ignored)."""
    import masked_sweep_cases as ms
    from tritd import drivers
    W = ms.mask(case)
    H = drivers.holdout_mask(W, 0.10, np.random.default_rng([case[1], 13]))
    H[:16, 3, :16] = True
    H[:16, 4, :16] = False
    H[:16, 1, 16:32] = True
    return np.asfortranarray(H)


def rank_selection_case():
    """tests/holdout_als_cases.rank_selection_case (35 x 22 x 36, planted rank
    3, 1 % noise, 30 % missing, candidates (2, 3, 5), 15 % of the observed
    entries held out) for the ADMM: the traffic options at 40 iterations and
    lambda in (1, 5) x sweep_cases.active_lambda(X).  The oracle's minimum
    valHist is 1.0e-2 at (3, 5 x), 3.3e-2 at r = 5 and 0.62 at r = 2, while the
    last errHist is smallest at r = 2 (tests/test_holdout_admm_oracle.py)."""
    import holdout_als_cases as hac
    import sweep_cases as sc
    from tritd import synth
    c = hac.rank_selection_case()
    lam = sc.active_lambda(c["X"])
    return dict(c, opts=dict(synth.TRAFFIC_OPTS, maxIter=40), lambdas=(lam, 5.0 * lam))
