"""Shared inputs of the masked rank sweep: tests/sweep_cases.e_active_case (an
ACTIVE outlier tensor E, ragged shapes (35 + r%3, 19 + r%5, 33 + r%4), lambda =
2e-3 std(D), 10 iterations) with an observation mask, for the CP model at every
rank r = 1..16 and the Qi model at r = 1..8.

The mask: 15 % of the entries missing at random (default_rng([r, 7])), and on
top of that
  * W[:16, 1, 16:32] = False: a whole 16 x 16 (i, t) tile of fibre j = 1 missing;
  * W[32:, 2, :16]  = False: every real row of a ragged edge tile missing (the
    tile holds padding rows beside real rows none of which is observed);
  * W[:16, 3, :16]  = True: a fully observed tile.

Reference: tests/masked_oracle.py, computed once per process and shared
(lru_cache); callers must not modify the arrays they get.  Tolerances: those of
tests/masked_cases.py, unchanged.  tests/test_masked_sweep_cases.py asserts (on
the CPU) that every case passes the admission rule of the masked goldens, that
E is active, and which cases mix compact slots with dense tiles.
"""
import functools

import numpy as np

import masked_oracle as mo
import sweep_cases as sc
from masked_cases import ATOL_ERR, MARGIN, TOL_ABC, TOL_ERR, TOL_LOE  # noqa: F401

ITERS = sc.ITERS
CASES = tuple(("cp", r) for r in range(1, 17)) + tuple(("qi", r) for r in range(1, 9))
# one rank per masked k5_fused instantiation: padded rank 16, 32, 48, 64, 128, 256
SCHEDULE_RANKS = (1, 5, 6, 7, 11, 13)
NARROW = (1, 5, 6, 7)  # padded rank <= 64: the side solve and the dense-E form
HIDDEN_RANKS = (3, 6, 11)
MISSING = 0.15
MISSING_BAND = (0.14, 0.18)
# nnz(E) / nnz(observed) of the reference after 3 and after ITERS iterations
NNZ3_MIN = 0.003
NNZ_BAND = (0.04, 0.75)
TILE_SHARE_MIN = 0.08
# nnz(E) is about 5 % on these and no 16 x 16 tile holds more than
# sweep_cases.TILE_CAP nonzeros: compact slots only
COMPACT_ONLY = (("cp", 2), ("cp", 4), ("qi", 3))
# the admission rule of tests/golden/make_masked_golden.py
PERTURB = 1e-15
PERTURB_SEEDS = (1, 2, 3)
# (every case passes the admission rule with sweep_cases' own data seed: there
# is no seed table here)


def case_id(case):
    return "%s-r%d" % case


def mask(case):
    """The observation mask of `case` (bool, column-major)."""
    model, r = case
    shape = sc.e_active_shape(r)
    W = np.random.default_rng([r, 7]).random(shape) >= MISSING
    W[:16, 1, 16:32] = False
    W[32:, 2, :16] = False
    W[:16, 3, :16] = True
    return np.asfortranarray(W)


def hidden_shard_mask(case, P=3):
    """mask(case) with rows 0 .. n1//P - 1 all False: shard 0 of a device set
    of P observes nothing while the other shards do."""
    W = mask(case).copy(order="F")
    W[:W.shape[0] // P] = False
    return W


def inputs(case, observed=None):
    """dict(D, A0, B0, C0, opts, r, observed, name): sweep_cases.e_active_case
    and the mask of a masked solve; `observed` replaces the case's own mask."""
    model, r = case
    c = sc.e_active_case(r, model=model)
    c["observed"] = mask(case) if observed is None else observed
    c["name"] = case_id(case)
    return c


def run_oracle(c, iters=ITERS, D=None, A0=None, B0=None, C0=None):
    t = mo.triple_decomp_ADMM_masked(c["D"] if D is None else D, c["observed"], c["r"],
                                     dict(c["opts"], maxIter=iters), c["A0"] if A0 is None else A0,
                                     c["B0"] if B0 is None else B0, c["C0"] if C0 is None else C0)
    return sc.as_ref(t)


@functools.lru_cache(maxsize=None)
def reference(case, iters=ITERS):
    """The masked oracle on inputs(case), as a dict like sweep_cases.as_ref."""
    return run_oracle(inputs(case), iters)


@functools.lru_cache(maxsize=None)
def hidden_reference(case, P=3):
    """The masked oracle on inputs(case) with hidden_shard_mask(case, P)."""
    return run_oracle(inputs(case, hidden_shard_mask(case, P)))


def golden_like(case, observed=None, ref=None):
    """Inputs and reference in one dict, the form test_gpu_masked.check_masked
    takes a golden in."""
    g = inputs(case, observed)
    g.update(reference(case) if ref is None else ref)
    return g


def nnz_of_observed(E, W):
    return np.count_nonzero(E) / np.count_nonzero(W)


def drifts(c, ref):
    """Worst change of every compared quantity when the oracle is rerun with D,
    A0, B0 and C0 perturbed by 1e-15 relative (make_masked_golden.drifts):
    dict(L, O, E, ABC, errHist_gate, k)."""
    import tritd_oracle as orc
    model = orc.opts_model(c["opts"])
    L = orc.triple_product(ref["A"], ref["B"], ref["C"], model)

    def rel(a, b):
        den = np.linalg.norm(np.ravel(b))
        return float(np.linalg.norm(np.ravel(a - b)) / (den if den > 0 else 1.0))

    out = dict(L=0.0, O=0.0, E=0.0, ABC=0.0, errHist_gate=0.0, k=0.0)
    for seed in PERTURB_SEEDS:
        rng = np.random.default_rng(seed)
        p = [np.asfortranarray(x * (1.0 + PERTURB * rng.standard_normal(x.shape)))
             for x in (c["D"], c["A0"], c["B0"], c["C0"])]
        q = run_oracle(c, len(ref["errHist"]), *p)
        out["k"] = max(out["k"], float(abs(q["k"] - ref["k"])))
        if q["k"] != ref["k"]:
            continue
        out["L"] = max(out["L"], rel(orc.triple_product(q["A"], q["B"], q["C"], model), L))
        out["O"] = max(out["O"], rel(q["O"], ref["O"]))
        out["E"] = max(out["E"], rel(q["E"], ref["E"]))
        for key in "ABC":
            out["ABC"] = max(out["ABC"], rel(q[key], ref[key]))
        eh, eh2 = ref["errHist"], q["errHist"]
        out["errHist_gate"] = max(out["errHist_gate"],
                                  float(np.max(np.abs(eh2 - eh) / (TOL_ERR * np.abs(eh) + ATOL_ERR))))
    return out
