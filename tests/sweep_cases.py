"""Shared inputs of the rank sweep (r = 1..16) with an ACTIVE outlier tensor E.

With the traffic driver's options (mu = 1e-3, lambda = 1.8, rho = 1.25) the
soft threshold lambda/mu starts at 1800 and shrinks by 1.25 per iteration,
while the synthetic outliers are ~10 r in size: E stays identically zero for
the first 12-20 iterations, and a short parity run compares an E that is all
zeros (the soft threshold, the compact-slot encode/decode, the overflow to
dense tiles, the dE chain behind O and the derived Y_O all degenerate to
no-ops).  The cases here set lambda = 2e-3 std(D), so the threshold starts at
2 std(D) and E is active from the first iterations; tests/test_sweep_cases.py
asserts (on the CPU) that every case really is active, mixed between the
compact and the dense tile forms, and well conditioned in fp64 and fp32.

Shapes (35 + r%3, 19 + r%5, 33 + r%4): every mode ragged against the 16-row
and 16-t tiles, more than one tile in i and in t.

One more case, TALL, stands beside the ranks wherever a function here takes a
case: 97 x 83 x 85 at r = 7 (padded rank 64; n1p = 112, n2 = 83, n3p = 96).
Every sweep shape keeps rows * RP^2 within the 327 680 up to which a factor's
apply and Gram are one launch (80 rows at RP = 64; csrc/kernels.h
apply_gram_small), so only this case takes the two-launch branch of all three
factor updates, and with it the side jobs without a deferred Gram.

References are computed once per process and shared (lru_cache); callers must
not modify the arrays they get.
"""
import functools
import os
import subprocess

import numpy as np

RANKS = tuple(range(1, 17))
ITERS = 10
# nnz(E) / E.size of the reference after 3 and after ITERS iterations
NNZ3_MIN = 0.005
NNZ_BAND = (0.10, 0.70)
# a 16 x 16 (i, t) tile of one fibre j with few nonzeros is kept as a compact
# slot, one with more is stored densely: up to 27 in fp64 (csrc/common.h
# CE_CAP), up to 56 in fp32 (k_admm32.hip).  Tiles with 1..TILE_CAP nonzeros
# are compact in fp32 and (but for a count of exactly 28) in fp64; tiles with
# more are dense in fp64.  The GPU sessions' dense-tile counters confirm both
# forms ran (tests/test_gpu_rank_sweep.py).
TILE_CAP = 28
TILE_SHARE_MIN = 0.10


TALL = "tall"
TALL_SHAPE, TALL_RANK = (97, 83, 85), 7


def e_active_shape(r):
    return (35 + r % 3, 19 + r % 5, 33 + r % 4)


def case_rank(case):
    """A case is a rank r of RANKS (at e_active_shape(r)) or TALL."""
    return TALL_RANK if case == TALL else case


def case_shape(case):
    return TALL_SHAPE if case == TALL else e_active_shape(case)


def active_lambda(D):
    """lambda with lambda/mu = 2 std(D) at TRAFFIC_OPTS' mu = 1e-3."""
    return 2e-3 * float(np.std(np.asarray(D, dtype=np.float64)))


# seed = r unless the case then misses a condition of tests/test_sweep_cases.py
# (Qi model, r = 6 and 7: nnz(E) 70.2 % and 71.2 % after 10 iterations with seed r)
_SEEDS = {("qi", 6): 46, ("qi", 7): 47}


@functools.lru_cache(maxsize=None)
def _case64(case, model):
    from tritd import synth
    r = case_rank(case)
    d = synth.low_rank_plus_outliers(*case_shape(case), r, seed=_SEEDS.get((model, case), r),
                                     init_seed=r + 100, model=model)
    opts = dict(synth.TRAFFIC_OPTS, maxIter=ITERS)
    opts["lambda"] = active_lambda(d["D"])
    if model != "cp":
        opts["model"] = model
    return d, opts


def e_active_case(case, dtype=np.float64, model="cp"):
    """dict(D, Lstar, A0, B0, C0, opts, r): D of `dtype` (column-major), lambda
    from the fp64 D for either dtype so both precisions solve the same problem;
    Lstar is the generator's low-rank part in fp64 (the driver's RRE reference)."""
    d, opts = _case64(case, model)
    return dict(D=np.asfortranarray(d["D"], dtype=dtype), Lstar=d["Lstar"], A0=d["A0"], B0=d["B0"],
                C0=d["C0"], opts=dict(opts), r=case_rank(case))


def as_ref(t):
    """Oracle / restatement tuple (A, B, C, O, errHist, E, k, ...) -> dict."""
    return dict(A=t[0], B=t[1], C=t[2], O=t[3], errHist=np.asarray(t[4]), E=t[5], k=int(t[6]))


@functools.lru_cache(maxsize=None)
def oracle_ref(case, model="cp", iters=ITERS):
    """The numpy oracle on e_active_case(case) (fp64)."""
    import tritd_oracle as orc
    c = e_active_case(case, model=model)
    return as_ref(orc.triple_decomp_ADMM(c["D"], c["r"], dict(c["opts"], maxIter=iters), c["A0"],
                                         c["B0"], c["C0"]))


@functools.lru_cache(maxsize=None)
def cref_lib():
    """The C restatement (oracle/tritd_ref.c), built on first use."""
    import tritd_oracle
    import tritd_ref
    here = os.path.dirname(os.path.abspath(tritd_oracle.__file__))
    subprocess.run(["make", "-C", here], check=True, capture_output=True)
    return tritd_ref, tritd_ref.load()


@functools.lru_cache(maxsize=None)
def c_ref(case, single, iters=ITERS):
    """The C restatement on e_active_case(case): class double or class single."""
    mod, lib = cref_lib()
    c = e_active_case(case, np.float32 if single else np.float64)
    return as_ref(mod.admm(lib, c["D"], c["r"], dict(c["opts"], maxIter=iters), c["A0"], c["B0"],
                           c["C0"]))


def nnz_share(E):
    return np.count_nonzero(E) / E.size


def tile_shares(E, cap=TILE_CAP):
    """(share of 16 x 16 (i, t) tiles of a fibre j with 1..cap nonzeros, share
    with more than cap), over all tiles including the ragged edge ones."""
    E = np.asarray(E)
    n1, n2, n3 = E.shape
    counts = []
    for i0 in range(0, n1, 16):
        for t0 in range(0, n3, 16):
            blk = E[i0:i0 + 16, :, t0:t0 + 16] != 0
            counts.append(blk.sum(axis=(0, 2)))  # one count per fibre j
    counts = np.concatenate(counts)
    return float(np.mean((counts >= 1) & (counts <= cap))), float(np.mean(counts > cap))


def perturbed(x, eps, rng):
    """x (1 + eps U(-1, 1)) elementwise, same dtype and memory order."""
    x = np.asarray(x)
    u = rng.uniform(-1.0, 1.0, size=x.shape)
    return np.asfortranarray((x.astype(np.float64) * (1.0 + eps * u)).astype(x.dtype))


# ---------------------------------------------------------------------------
# the other solvers at the same ragged shapes
# ---------------------------------------------------------------------------
ALS_OPTS = dict(maxIter=8, tol=0.0)
# parameters of the committed nc*.npz goldens (tests/golden/make_golden.py)
NCVX_PARAMS = dict(rho=1.0, lam=0.5, gamma_A=1e-3, epsilon=1e-2, p=0.5, theta=2.0 / 3.0,
                   maxIter=8, tol=0.0)


def ncvx_args(prm=None):
    p = dict(NCVX_PARAMS, **(prm or {}))
    return [p[k] for k in ("rho", "lam", "gamma_A", "epsilon", "p", "theta", "maxIter", "tol")]


def oracle_als(r, X=None, A0=None):
    """Oracle ALS on e_active_case(r)'s D (or a perturbed X / A0): (A, B, C, errHist, k)."""
    import tritd_oracle as orc
    c = e_active_case(r)
    return orc.triple_decomp_ALS(c["D"] if X is None else X, r, ALS_OPTS,
                                 c["A0"] if A0 is None else A0, c["B0"], c["C0"],
                                 printer=lambda s: None)


def oracle_ncvx(r, X=None, A0=None):
    """Oracle nonconvex solver on e_active_case(r)'s D: (A, B, C, O, errHist, k, trace)."""
    import tritd_oracle as orc
    c = e_active_case(r)
    return orc.triple_decomp_ADMM_ncvx(c["D"] if X is None else X, r, *ncvx_args(),
                                       c["A0"] if A0 is None else A0, c["B0"], c["C0"],
                                       printer=lambda s: None)


oracle_als_ref = functools.lru_cache(maxsize=None)(lambda r: oracle_als(r))
oracle_ncvx_ref = functools.lru_cache(maxsize=None)(lambda r: oracle_ncvx(r))
