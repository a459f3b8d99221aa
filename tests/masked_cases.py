"""The goldens of the mask-aware ADMM (tests/golden/m*.npz) and what each is
held to.  Shared by tests/test_masked_oracle.py (CPU) and
tests/test_gpu_masked.py (GPU).

Tolerances are those of tests/test_gpu_parity.py.  A golden is held to a
tolerance only where its stored drift (tests/golden/make_masked_golden.py: the
oracle rerun with inputs perturbed by 1e-15 relative) is at least 100x below
it; `held()` lists, per golden, the quantities that pass this rule, and the
CPU suite asserts that they do.
"""
import glob
import os

from conftest import GOLDEN, load_golden

TOL_LOE = 1e-9    # L, O, E: relative Frobenius
TOL_ABC = 1e-8    # A, B, C
TOL_ERR = 1e-8    # errHist: |d| <= TOL_ERR |ref| + ATOL_ERR
ATOL_ERR = 1e-11
TOL_IT12 = 1e-11  # A, B, C after iterations 1 and 2
MARGIN = 100.0

# quantity -> (name of the stored drift, the tolerance it is compared at)
QUANTITIES = {
    "L": ("drift_L", TOL_LOE),
    "O": ("drift_O", TOL_LOE),
    "E": ("drift_E", TOL_LOE),
    "O_normD": ("drift_O_normD", TOL_LOE),  # ||O - O_ref|| / ||Omega o D||
    "E_normD": ("drift_E_normD", TOL_LOE),
    "ABC": ("drift_ABC", TOL_ABC),
    "errHist": ("drift_errHist_gate", 1.0),  # stored in units of the gate itself
    "it12": ("drift_it12_ABC", TOL_IT12),
}
DEFAULT = ("L", "O", "E", "ABC", "errHist", "it12")
# The sensor-like case: ||O|| is small there (O and E are measured against
# ||Omega o D||), the factors after iterations 1 and 2 drift by 3.8e-13 (above
# 1e-11 / 100), and at 20 iterations A, B, C drift by 1.8e-10 (above 1e-8 /
# 100) while L does not; the 14-iteration golden holds A, B, C.
SPECIAL = {
    "m54x4x96_r5_sensor": ("L", "O_normD", "E_normD", "errHist"),
    "m54x4x96_r5_sensor_k14": ("L", "O_normD", "E_normD", "ABC", "errHist"),
}


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "m*.npz")))


def load(name):
    g = load_golden(name)
    g["observed"] = g["observed"].astype(bool)
    return g


def held(name):
    return SPECIAL.get(name, DEFAULT)
