"""Generate the golden vectors of the mask-aware nonconvex solver
(tests/golden/onc*.npz).

The vectors come from tests/masked_ncvx_oracle.py (the restatement of
fast_robust_triple_tensor/test.m:1-73 with an observation mask).  Run from the
repo root:

    python tests/golden/make_masked_ncvx_golden.py [name ...]

Each .npz holds the inputs (X, observed, A0, B0, C0, r, the eight parameters
of test.m:1 as JSON in `opts`) and the outputs (A, B, C, O, errHist, k).
onc12x10x8_r2 also holds the state after iterations 1 and 2 (it1_*, it2_*:
A, B, C, O = O_new, Lam, Gam).  Three cases take the inputs of the committed
nc*.npz goldens of the unmasked solver; onc20x6x70_r3 (five t-tiles) draws its
own with the generator and parameters of those (tests/golden/make_golden.py).

Admission rule (that of make_masked_als_golden.py).  The oracle is also rerun
with X, A0, B0 and C0 perturbed by 1e-15 relative (three seeds), and the worst
drift of every compared quantity is stored (drift_*).  A case is held to a
tolerance only if its stored drift is at least 100x below that tolerance
(tests/test_masked_ncvx_oracle.py asserts it for every file).  A case that
fails the rule gets a shorter maxIter, never a looser tolerance.
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

import masked_ncvx_cases as mnc  # noqa: E402
import masked_ncvx_oracle as mno  # noqa: E402
from conftest import load_golden  # noqa: E402

MASK_SEED = 11
NCVX_PARAMS = dict(rho=1.0, **{"lambda": 0.5}, gamma_A=1e-3, epsilon=1e-2, p=0.5, theta=2.0 / 3.0)


def random_mask(shape, missing, seed=MASK_SEED):
    return np.random.default_rng(seed).random(shape) >= missing


def three_tiles(shape):
    """15 % missing at random and, on top: a wholly missing 16 x 16 (i, t) tile
    of fibre j = 1, a ragged edge tile (rows 16..29 real, 30..31 padding) of
    fibre j = 2 with no observed real row, a fully observed tile of j = 3."""
    W = random_mask(shape, 0.15)
    W[:16, 1, 16:32] = False
    W[16:, 2, :16] = False
    W[:16, 3, :16] = True
    return W


def from_golden(name):
    g = load_golden(name)
    return dict(X=g["X"], A0=g["A0"], B0=g["B0"], C0=g["C0"]), g["r"], dict(g["opts"])


def drawn(n1, n2, n3, r, prm):
    from tritd import synth
    d = synth.low_rank_plus_outliers(n1=n1, n2=n2, n3=n3, r=r)
    return dict(X=d["D"], A0=d["A0"], B0=d["B0"], C0=d["C0"]), r, prm


# name: (inputs, mask of the inputs' shape, changes to the parameters)
CASES = {
    # a single ragged tile, one t-tile; the state after iterations 1 and 2
    "onc12x10x8_r2": (lambda: from_golden("nc12x10x8_r2"), lambda s: random_mask(s, 0.30), {}),
    # the stop test of :65 fires before maxIter: errHist truncated, O of iteration k-1
    "onc20x24x18_r3_stop": (lambda: from_golden("nc20x24x18_r3_stop"),
                            lambda s: random_mask(s, 0.15, seed=5), {}),
    # a wholly missing tile, an edge tile with no observed real row, a fully observed tile
    "onc30_r3_tiles": (lambda: from_golden("nc30_r3"), three_tiles, dict(maxIter=12)),
    # 5 t-tiles: the paired walk plus a remainder
    "onc20x6x70_r3": (lambda: drawn(20, 6, 70, 3, dict(NCVX_PARAMS, maxIter=10, tol=0.0)),
                      lambda s: random_mask(s, 0.30), {}),
}
TRACED = {"onc12x10x8_r2": (1, 2)}


def case_inputs(name):
    gen, mask, over = CASES[name]
    d, r, prm = gen()
    prm = dict(prm, **over)
    return d, np.asfortranarray(mask(d["X"].shape)), r, prm


def make(name):
    d, observed, r, prm = case_inputs(name)
    a = [prm[k] for k in mnc.PARAM_KEYS]
    ref = mno.triple_decomp_ncvx_masked(d["X"], observed, r, *a, d["A0"], d["B0"], d["C0"],
                                        printer=mnc.quiet, trace_iters=TRACED.get(name, ()))
    A, B, C, O, eh, k, trace = ref
    out = dict(X=d["X"], observed=observed, A0=d["A0"], B0=d["B0"], C0=d["C0"], r=np.int64(r),
               opts=np.array(json.dumps(prm)), A=A, B=B, C=C, O=O, errHist=eh, k=np.int64(k))
    for it, st in trace.items():
        for key, v in st.items():
            out["it%d_%s" % (it, key)] = v
    dr = mnc.drifts(ref, d["X"], observed, r, a, d["A0"], d["B0"], d["C0"])
    for key, v in dr.items():
        out["drift_" + key] = np.float64(v)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    return k, eh, dr


if __name__ == "__main__":
    for n in (sys.argv[1:] or CASES):
        k, eh, dr = make(n)
        print(n, "k=%d errHist[0]=%.3e errHist[-1]=%.3e" % (k, eh[0], eh[-1]),
              " ".join("%s=%.1e" % kv for kv in dr.items()))
