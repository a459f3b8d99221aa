"""The goldens of the mask-aware ALS (tests/golden/oals*.npz) and what each is
held to.  Shared by tests/test_masked_als_oracle.py (CPU) and
tests/test_gpu_masked_als.py (GPU).

Tolerances are those of tests/test_gpu_als.py.  A golden is held to a
tolerance only where its stored drift (tests/golden/make_masked_als_golden.py:
the oracle rerun with inputs perturbed by 1e-15 relative) is at least 100x
below it (the rule of tests/masked_cases.py); `held()` lists, per golden, the
quantities that pass this rule, and the CPU suite asserts that they do.  Every
golden is held for L and errHist, and every padded rank (16, 32, 48, 64) has
at least one golden held for A, B, C.
"""
import glob
import os

import numpy as np

from conftest import GOLDEN, load_golden

TOL_ABC = 1e-8    # A, B, C: relative Frobenius
TOL_L = 1e-9      # triple_product(A, B, C)
TOL_ERR = 1e-9    # errHist: relative
ATOL_ERR = 1e-14
MARGIN = 100.0

# quantity -> (name of the stored drift, the tolerance it is compared at)
QUANTITIES = {
    "L": ("drift_L", TOL_L),
    "ABC": ("drift_ABC", TOL_ABC),
    "errHist": ("drift_errHist", TOL_ERR),
}
DEFAULT = ("L", "ABC", "errHist")
# goldens whose factors drift by more than TOL_ABC / 100 while L does not
# (the factors of a triple decomposition are less well determined than their
# product): held for L and errHist only
SPECIAL = {}


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "oals*.npz")))


def load(name):
    g = load_golden(name)
    g["observed"] = g["observed"].astype(bool)
    return g


def held(name):
    return SPECIAL.get(name, DEFAULT)


def padded_rank(r):
    return (r * r + 15) // 16 * 16


NOISE = 0.01  # of std(L*)


def noisy_low_rank(n1, n2, n3, r, seed=0):
    """dict(X, Lstar, A0, B0, C0): L* of synth.low_rank_plus_outliers without
    outliers plus N(0, (1 % std)^2) noise — what an ALS completion user fits."""
    from tritd import synth
    d = synth.low_rank_plus_outliers(n1, n2, n3, r, p_out=0.0, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    X = d["Lstar"] + NOISE * float(d["Lstar"].std()) * rng.standard_normal(d["Lstar"].shape)
    return dict(X=np.asfortranarray(X), Lstar=d["Lstar"], A0=d["A0"], B0=d["B0"], C0=d["C0"])


def completion_case():
    """The rank sweep's r = 3 inputs (tests/sweep_cases.py: 35 x 22 x 36) without
    their outliers, 1 % noise, 30 % missing, 40 iterations: the masked fit
    against the zero-filled one.  The oracles leave a relative error on the
    missing entries of 2.2e-3 (masked) and 0.34 (zero fill)."""
    import sweep_cases as sc
    c = sc.e_active_case(3)
    rng = np.random.default_rng(2003)
    X = np.asfortranarray(c["Lstar"] + NOISE * np.std(c["Lstar"]) * rng.standard_normal(c["Lstar"].shape))
    observed = np.asfortranarray(rng.random(X.shape) >= 0.30)
    d = dict(X=X, Lstar=c["Lstar"], A0=c["A0"], B0=c["B0"], C0=c["C0"])
    return d, observed, 3, dict(maxIter=40, tol=0.0)
