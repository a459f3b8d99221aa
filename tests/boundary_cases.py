"""Shared inputs of tests/test_gpu_session_boundary.py: what a caller hands to
a Session (D with a leading dimension, a pointer into a larger tensor) and the
reference tensors of tritd_session_rre_parts.

Cases (kind, key):
  ("cp", r)   sweep_cases.e_active_case(r), r in RANKS: one rank per padded
              rank 16, 32, 48, 64, 128, 256
  ("f32", r)  the same inputs with a float32 D, r in F32_RANKS
  ("qi", r)   sweep_cases.e_active_case(r, model="qi"), r in QI_RANKS
  ("deg", q)  DEGENERATE[q]: the shapes of test_gpu_parity.DEGENERATE with a
              singleton mode, from synth.low_rank_plus_outliers, E active
Every case runs STEPS = 3 + 7 iterations.

Buffer forms (FORMS): how the shard's rows sit in the caller's buffer —
"contig" (ld = n1), "strided" (ld = n1 + 3) and "offset" (ld = n1 + 5, the
shard at rows 3..3+n1-1: the pointer is advanced by an odd number of
elements).  Every element outside the shard's rows is NaN, so one padded
element read shows in any sum or iterate.

References are computed once per process (lru_cache); callers must not modify
the arrays they get.  tests/test_boundary_cases.py asserts on the CPU that
these inputs are what the GPU module takes them for.
"""
import functools

import numpy as np

import sweep_cases as sc

RANKS = (4, 5, 6, 8, 11, 16)
F32_RANKS = (4, 16)
QI_RANKS = (2, 5, 8)
DEGENERATE = (((5, 1, 7), 2), ((1, 9, 8), 2), ((33, 17, 1), 3))
STEPS = (3, 7)
ITERS = sum(STEPS)
assert ITERS == sc.ITERS

# form -> (rows of the buffer beyond n1, row of the buffer the shard starts at)
FORMS = {"contig": (0, 0), "strided": (3, 0), "offset": (5, 3)}

CASES = ([("cp", r) for r in RANKS] + [("f32", r) for r in F32_RANKS] + [("qi", r) for r in QI_RANKS]
         + [("deg", q) for q in range(len(DEGENERATE))])

# tritd_session_rre_parts against numpy (tests/test_gpu_session_boundary.py):
# den is a fixed-order sum of squares, the suite's tolerance for those against
# numpy (tests/test_gpu_metrics.py); num = sum (L - X)^2 moves by about
# 2 <L - X, dL> when the MFMA product L moves by dL, |dL| <= TOL_TP |L|
# (the tolerance tests/test_gpu_parity.py::test_triple_product holds the same
# product to), so by at most 2 TOL_TP |L| / |L - X| relative.
RTOL_SUM = 1e-12
TOL_TP = 1e-13
# X1, X2 are far from L: their num tolerance stays at or below 3e-12
FAR = 0.1
X3_EPS = 1e-6


def case_id(case):
    return "%s%s" % (case[0], case[1] if case[0] != "deg" else "x".join(map(str, DEGENERATE[case[1]][0])))


# A rank-r^2 model fits most of a 35-element tensor, outliers included: with
# 30 % outliers and these seeds E is active (nnz >= 20 % after ITERS
# iterations, the bar of test_gpu_parity's degenerate cases; asserted by
# tests/test_boundary_cases.py).  5 x 1 x 7 reaches it with 2 seeds of 20..39.
_DEG_P_OUT = 0.3
_DEG_SEEDS = (38, 21, 22)


@functools.lru_cache(maxsize=None)
def _degenerate64(q):
    from tritd import synth
    shape, r = DEGENERATE[q]
    d = synth.low_rank_plus_outliers(*shape, r, p_out=_DEG_P_OUT, seed=_DEG_SEEDS[q],
                                     init_seed=120 + q)
    opts = dict(synth.TRAFFIC_OPTS, maxIter=ITERS)
    opts["lambda"] = sc.active_lambda(d["D"])
    return d, opts


def inputs(case):
    """dict(D, Lstar, A0, B0, C0, opts, r, model, f32) of a case; D float32
    for the "f32" kind, Lstar always float64."""
    kind, key = case
    if kind == "deg":
        d, opts = _degenerate64(key)
        c = dict(D=d["D"], Lstar=d["Lstar"], A0=d["A0"], B0=d["B0"], C0=d["C0"], opts=dict(opts),
                 r=DEGENERATE[key][1])
    else:
        c = sc.e_active_case(key, np.float32 if kind == "f32" else np.float64,
                             model="qi" if kind == "qi" else "cp")
    c["model"] = "qi" if kind == "qi" else "cp"
    c["f32"] = kind == "f32"
    return c


@functools.lru_cache(maxsize=None)
def reference(case):
    """The solve of a case after ITERS iterations: the numpy oracle (fp64
    kinds) or the class-single C restatement ("f32")."""
    import tritd_oracle as orc
    kind, key = case
    if kind == "cp":
        return sc.oracle_ref(key)
    if kind == "qi":
        return sc.oracle_ref(key, model="qi")
    if kind == "f32":
        return sc.c_ref(key, True)
    c = inputs(case)
    return sc.as_ref(orc.triple_decomp_ADMM(c["D"], c["r"], c["opts"], c["A0"], c["B0"], c["C0"]))


@functools.lru_cache(maxsize=None)
def reference_product(case, fresh):
    """triple_product of the reference's factors after ITERS iterations, or
    (fresh) of the initial factors: what a session holds before any run."""
    import tritd_oracle as orc
    c = inputs(case)
    f = (c["A0"], c["B0"], c["C0"]) if fresh else tuple(reference(case)[k] for k in "ABC")
    return orc.triple_product(*f, model=c["model"])


@functools.lru_cache(maxsize=None)
def rre_tensors(case, fresh):
    """(X1, X2, X3) of a case, column-major, float32 for the "f32" kind:
    X1 = Lstar (the driver's call), X2 an independent normal tensor scaled to
    std(D) (no cancellation), X3 = L (1 + 1e-6 U(-1, 1)) around the
    reference's product (the near-converged regime of the bench line, where
    num is a difference of nearly equal numbers)."""
    c = inputs(case)
    dt = np.float32 if c["f32"] else np.float64
    rng = np.random.default_rng([CASES.index(case), int(fresh), 7])
    D64 = np.asarray(c["D"], np.float64)
    X2 = rng.standard_normal(D64.shape) * float(np.std(D64))
    L = reference_product(case, fresh)
    X3 = L * (1.0 + X3_EPS * rng.uniform(-1.0, 1.0, size=L.shape))
    return tuple(np.asfortranarray(x, dtype=dt) for x in (c["Lstar"], X2, X3))


def rre_reference(L, X):
    """(num, den, rtol of num, rtol of den) of sum (L - X)^2 and sum X^2 in
    float64 (X widened exactly); the tolerances from the reference alone."""
    L = np.asarray(L, np.float64)
    X = np.asarray(X, np.float64)
    d = (L - X).ravel()
    x = X.ravel()
    num, den = float(np.dot(d, d)), float(np.dot(x, x))
    ratio = float(np.linalg.norm(L.ravel())) / np.sqrt(num)
    return num, den, RTOL_SUM + 2.0 * TOL_TP * ratio, RTOL_SUM


def padded(X, form, fill=np.nan):
    """(buffer, ld, off): X's rows inside a column-major buffer of FORMS[form],
    `fill` everywhere else; X(i,j,t) sits at flat element off + i + ld (j + n2 t)."""
    X = np.asarray(X)
    extra, off = FORMS[form]
    n1 = X.shape[0]
    buf = np.full((n1 + extra,) + X.shape[1:], fill, dtype=X.dtype, order="F")
    buf[off:off + n1] = X
    return buf, n1 + extra, off


# ---------------------------------------------------------------------------
# a proper sub-range of the rows without a communicator: Session::allreduce
# returns at once, so the session solves D[i0:i1], A0[i0:i1], B0, C0 on its own
# ---------------------------------------------------------------------------
SUB_RANKS = (4, 11)


def sub_range(n1):
    """rows 5 .. n1-5: straddles the 16-row tiles at both ends"""
    return 5, n1 - 4


@functools.lru_cache(maxsize=None)
def sub_reference(r):
    import tritd_oracle as orc
    c = sc.e_active_case(r)
    i0, i1 = sub_range(c["D"].shape[0])
    return sc.as_ref(orc.triple_decomp_ADMM(np.asfortranarray(c["D"][i0:i1]), r, c["opts"],
                                            np.asfortranarray(c["A0"][i0:i1]), c["B0"], c["C0"]))
