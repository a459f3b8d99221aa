"""The goldens of the mask-aware nonconvex solver (tests/golden/onc*.npz), the
masked rank sweep and the completion case, and what each is held to.  Shared
by tests/test_masked_ncvx_oracle.py (CPU) and tests/test_gpu_masked_ncvx.py
(GPU).

Tolerances are those of tests/test_ncvx.py.  A quantity is held to its
tolerance only where the stored drift (tests/golden/make_masked_ncvx_golden.py:
the oracle rerun with X, A0, B0 and C0 perturbed by 1e-15 relative) is at least
100x below it (the rule of tests/masked_als_cases.py); `held()` lists, per
golden, the quantities that pass this rule, and the CPU suite asserts that they
do.

References are computed once per process and shared (lru_cache); callers must
not modify the arrays they get.
"""
import functools
import glob
import os

import numpy as np

import masked_ncvx_oracle as mno
import masked_sweep_cases as msc
import sweep_cases as sc
from conftest import GOLDEN, load_golden

TOL = 1e-9        # A, B, C, O and triple_product(A, B, C): relative Frobenius
RTOL_ERR = 1e-8   # errHist
ATOL_ERR = 1e-13
TOL_TRACE = 1e-11  # the state after iterations 1 and 2
MARGIN = 100.0

PARAM_KEYS = ("rho", "lambda", "gamma_A", "epsilon", "p", "theta", "maxIter", "tol")
NCVX_KEYS = ("rho", "lam", "gamma_A", "epsilon", "p", "theta")

# quantity -> (name of the stored drift, the tolerance it is compared at)
QUANTITIES = {
    "L": ("drift_L", TOL),
    "O": ("drift_O", TOL),
    "ABC": ("drift_ABC", TOL),
    "errHist": ("drift_errHist", RTOL_ERR),
}
DEFAULT = ("L", "O", "ABC", "errHist")
SPECIAL = {}  # (every golden passes the rule for every quantity)

SWEEP_RANKS = tuple(range(1, 9))
SWEEP_ITERS = 8
O_ACTIVE_BAND = (0.10, 0.99)  # nnz(O) / nnz(observed) of the sweep references


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "onc*.npz")))


def load(name):
    g = load_golden(name)
    g["observed"] = g["observed"].astype(bool)
    return g


def held(name):
    return SPECIAL.get(name, DEFAULT)


def padded_rank(r):
    return (r * r + 15) // 16 * 16


def args(g, **over):
    """The eight positional parameters of test.m:1 after (X, r), from a golden."""
    o = dict(g["opts"], **over)
    return [o[k] for k in PARAM_KEYS]


def ncvx_dict(prm):
    """args() -> the ncvx= dictionary of tritd.AlsSession."""
    return dict(zip(NCVX_KEYS, prm[:6]))


def rel(a, b):
    den = np.linalg.norm(np.ravel(b))
    return float(np.linalg.norm(np.ravel(a - b)) / (den if den > 0 else 1.0))


def quiet(s):
    pass


def drifts(ref, X, observed, r, prm, A0, B0, C0, perturb=1e-15, seeds=(1, 2, 3)):
    """Worst change of every compared quantity when the oracle is rerun with
    X, A0, B0 and C0 perturbed by 1e-15 relative: dict(L, O, ABC, errHist, k)."""
    import tritd_oracle as orc
    A, B, C, O, eh, k = ref[:6]
    L = orc.triple_product(A, B, C)
    out = dict(L=0.0, O=0.0, ABC=0.0, errHist=0.0, k=0.0)
    for seed in seeds:
        rng = np.random.default_rng(seed)
        p = [np.asfortranarray(x * (1.0 + perturb * rng.standard_normal(x.shape)))
             for x in (X, A0, B0, C0)]
        q = mno.triple_decomp_ncvx_masked(p[0], observed, r, *prm, p[1], p[2], p[3], printer=quiet)
        out["k"] = max(out["k"], float(abs(q[5] - k)))
        if q[5] != k:
            continue
        out["L"] = max(out["L"], rel(orc.triple_product(q[0], q[1], q[2]), L))
        out["O"] = max(out["O"], rel(q[3], O))
        for x2, x in zip(q[:3], (A, B, C)):
            out["ABC"] = max(out["ABC"], rel(x2, x))
        out["errHist"] = max(out["errHist"], float(np.max(np.abs(q[4] - eh) / np.abs(eh))))
    return out


# ---------------------------------------------------------------------------
# the rank sweep: sweep_cases.e_active_case(r) with masked_sweep_cases.mask
# ---------------------------------------------------------------------------
def sweep_inputs(r, observed=None):
    c = sc.e_active_case(r)
    c["observed"] = msc.mask(("cp", r)) if observed is None else observed
    return c


def sweep_args():
    return sc.ncvx_args(dict(maxIter=SWEEP_ITERS))


def as_ref(t):
    return dict(A=t[0], B=t[1], C=t[2], O=t[3], errHist=np.asarray(t[4]), k=int(t[5]))


@functools.lru_cache(maxsize=None)
def sweep_reference(r, hidden=0):
    """The masked oracle on the sweep inputs (hidden = P: with shard 0 of P
    observing nothing, masked_sweep_cases.hidden_shard_mask)."""
    c = sweep_inputs(r, msc.hidden_shard_mask(("cp", r), hidden) if hidden else None)
    return as_ref(mno.triple_decomp_ncvx_masked(c["D"], c["observed"], r, *sweep_args(), c["A0"],
                                                c["B0"], c["C0"], printer=quiet))


def completion_case():
    """masked_als_cases.completion_case() (35 x 22 x 36, r = 3, 1 % noise, 30 %
    missing) with the parameters of sweep_cases.NCVX_PARAMS for 20 iterations:
    the masked fit against the zero-filled one.  The oracles leave a relative
    error on the missing entries of 4.5e-3 (masked) and 0.337 (zero fill)."""
    import masked_als_cases as mac
    d, observed, r, _ = mac.completion_case()
    return d, observed, r, sc.ncvx_args(dict(maxIter=20))


COMPLETION_MAX = 1e-2    # masked error on the missing entries
COMPLETION_GAIN = 20.0   # and at least this many times below the zero fill
