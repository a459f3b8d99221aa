"""Shared inputs of the option ladder (tests/test_opts_cases.py on the CPU,
tests/test_gpu_opts_ladder.py on the GPU).

Every other parity test of the robust ADMM runs at the traffic driver's
mu = 1e-3, rho = 1.25, lambda2 = 1e-3 (the K5 step cases at rho = 1.05, the
video configuration at mu = 1e-2, rho = 1.2), and the nonconvex solver at
sweep_cases.NCVX_PARAMS and two neighbours.  The fused fp64 update derives its
scalars from the mu schedule (invL, thr, rden, invL_next = 1/mu_[k], muO_prev =
mu_[k-2], cprev = muO_prev/mu_[k-1]: csrc/solver.cpp Session::scalars), so at
rho = 1.25 over 10 iterations cprev is always exactly 0.8 and the clip of
mu <- min(mu rho, 1e6 mu0) never acts.  The ladder below moves one option at a
time, on the sweep's inputs (sweep_cases.e_active_case: ragged 35 x 20 x 33
shapes) with the sweep's lambda rule, lambda = 2 std(D) mu (threshold
lambda/mu = 2 std(D) in the first iteration), unless the regime sets lambda.

References are computed once per process and shared (lru_cache); callers must
not modify the arrays they get.
"""
import functools

import numpy as np

import k5_step_bits_cases as kc
import sweep_cases as sc

# regime id -> (overrides, iterations).  An override "lambda_std": x sets
# lambda = x std(D); every other key replaces that option.
REGIMES = {
    "rho1": (dict(rho=1.0), 10),                          # cprev = 1, invL_next = invL
    "rho1_lam1": (dict(rho=1.0, lambda_std=1e-3), 10),    # tiles overflow, then return to a slot
    "rho_dec": (dict(rho=0.8), 10),                       # cprev = 1.25, Y_L/mu growing in the O fix-up
    "sat_fast": (dict(rho=1e6), 6),                       # saturated from iteration 2
    "sat_mid": (dict(rho=10.0), 10),                      # reaches 1e6 mu0 exactly at iteration 7
    "sat_clip": (dict(rho=4.0), 13),                      # 4^10 > 1e6: the one step the clip shortens
    "mu_small": (dict(mu=1e-7), 10),
    "mu_large": (dict(mu=10.0), 10),
    "mu1_rho1": (dict(mu=1.0, rho=1.0), 10),              # every scalar exactly 1 or 0.5
    "lam2_zero": (dict(lambda2=0.0), 10),                 # unregularised A and B Grams
    "lam2_big": (dict(lambda2=10.0), 10),                 # ridge dominating the Gram
    "lam_zero": ({"lambda": 0.0}, 10),                    # E = R3: every tile dense from iteration 1
    "lam_huge": ({"lambda": 1e30}, 10),                   # E identically zero, thr finite in single
}
IDS = tuple(REGIMES)
SATURATING = ("sat_fast", "sat_mid", "sat_clip")
# the regimes that also run the side-stream schedule, the forced dense-E form,
# a device set and the Qi model
SUBSET = ("rho1", "rho1_lam1", "rho_dec", "sat_clip", "lam_zero")
RANKS = (5, 8, 11)       # padded rank 32 (fused), 64 (the benchmark's), 128 (side-stream)
R_FORMS = 5              # sessions, masked, schedules, Qi
R_DEVICE_SET = 6
RANKS32 = (4, 16)
OBSERVED = kc.OBSERVED   # 70 % of the entries observed
# the 1e-14 response bounds of the CPU admission: 100x under TOL_LOE / TOL_ABC
RESPONSE_LOE = 1e-11
RESPONSE_ABC = 1e-10

# fp64 cells (regime, rank, model) whose reference misses RESPONSE_* and that
# the GPU module therefore leaves out (at most two; none measured)
DROPPED64 = ()


def iters(regime):
    return REGIMES[regime][1]


def schedule(regime):
    """mu_1 .. mu_{iters+1} of the regime (tritd_oracle.mu_schedule)."""
    import tritd_oracle as orc
    from tritd import synth
    o = dict(synth.TRAFFIC_OPTS, **{k: v for k, v in REGIMES[regime][0].items()
                                    if k in ("mu", "rho")})
    return np.asarray(orc.mu_schedule(o["mu"], o["rho"], iters(regime) + 1))


def case(regime, r, dtype=np.float64, model="cp", n=None):
    """sweep_cases.e_active_case(r) with the regime's options and iteration
    count (or n iterations)."""
    c = sc.e_active_case(r, dtype, model)
    over = dict(REGIMES[regime][0])
    lam_std = over.pop("lambda_std", None)
    opts = dict(c["opts"], **over)
    std = sc.active_lambda(sc.e_active_case(r, model=model)["D"]) / 2e-3  # std of the fp64 D
    if lam_std is not None:
        opts["lambda"] = lam_std * std
    elif "lambda" not in over:
        opts["lambda"] = 2.0 * std * opts["mu"]
    opts["maxIter"] = iters(regime) if n is None else n
    c["opts"] = opts
    return c


@functools.lru_cache(maxsize=None)
def ref(regime, r, model="cp", n=None):
    """The numpy oracle on case(regime, r)."""
    import tritd_oracle as orc
    c = case(regime, r, model=model, n=n)
    return sc.as_ref(orc.triple_decomp_ADMM(c["D"], c["r"], c["opts"], c["A0"], c["B0"], c["C0"]))


@functools.lru_cache(maxsize=None)
def observed(r):
    """The mask of the masked forms: OBSERVED of the entries, drawn as in k5_step_bits_cases."""
    return np.asfortranarray(np.random.default_rng([r, 11]).random(sc.e_active_shape(r)) < OBSERVED)


@functools.lru_cache(maxsize=None)
def masked_ref(regime, r, n=None):
    import masked_oracle as mo
    c = case(regime, r, n=n)
    return sc.as_ref(mo.triple_decomp_ADMM_masked(c["D"], observed(r), c["r"], c["opts"], c["A0"],
                                                  c["B0"], c["C0"]))


@functools.lru_cache(maxsize=None)
def c_ref32(regime, r):
    """The class-single C restatement on case(regime, r, float32)."""
    mod, lib = sc.cref_lib()
    c = case(regime, r, np.float32)
    return sc.as_ref(mod.admm(lib, c["D"], c["r"], c["opts"], c["A0"], c["B0"], c["C0"]))


def e_per_iteration(c, n, obs=None):
    """E of the oracle after each of the iterations 1..n of the case c."""
    import tritd_oracle as orc
    o = dict(c["opts"], maxIter=n)
    if obs is not None:
        import masked_oracle as mo
        t = mo.triple_decomp_ADMM_masked(c["D"], obs, c["r"], o, c["A0"], c["B0"], c["C0"],
                                         trace_iters=range(1, n + 1))
    else:
        t = orc.triple_decomp_ADMM(c["D"], c["r"], o, c["A0"], c["B0"], c["C0"],
                                   trace_iters=range(1, n + 1))
    assert t[6] == n
    return [t[7][k]["E"] for k in range(1, n + 1)]


# ---------------------------------------------------------------------------
# fp32: the cells (regime, rank) admitted by tests/test_opts_cases.py
# ---------------------------------------------------------------------------
# Rule of tests/test_sweep_cases.py: a cell is compared on the GPU only if the
# class-single restatement moves by at most a quarter of test_gpu_f32.TOL
# (5e-6) on L, O and E when D and A0 are perturbed by relative 2^-24 U(-1, 1),
# three seeds.  Measured responses (those in brackets are left out):
#              r = 4     r = 16
#   rho1       7.7e-7   [1.0e-5]   E all but empty at r = 16 (nnz 0.1 %), like
#   mu1_rho1   7.2e-7   [1.0e-5]   rho_dec: the few entries at the threshold
#   rho_dec    1.3e-6   [8.6e-6]   flip with the rounding of the inputs
#   rho1_lam1  8.4e-7   [4.7e-6]   under the bar by 7 %: left out, the margin is
#                                  less than a change of summation order moves it
#   sat_fast   1.5e-7    4.1e-7
#   sat_mid    1.7e-7    5.4e-7
#   sat_clip   1.8e-7    6.7e-7
#   mu_small   1.2e-7    2.3e-6
#   mu_large   1.3e-7    2.3e-6
#   lam2_zero  1.2e-7    2.2e-6
#   lam2_big   1.3e-7    2.2e-6
#   lam_zero   1.9e-7    4.3e-7
#   lam_huge   4.2e-7    3.0e-6
F32_RESPONSE_MAX = 5e-6
F32_ADMITTED = {
    4: IDS,
    16: tuple(g for g in IDS if g not in ("rho1", "mu1_rho1", "rho_dec", "rho1_lam1")),
}
# At r = 16 the class-single restatement takes 1.4 s per iteration on the host
# (R = 256): 14 s for a GPU test's reference, a minute for a cell's admission
# (four solves).  All nine admitted r = 16 cells passed on an MI355X
# (tests/test_gpu_opts_ladder.py lists their figures); the suite keeps the three
# whose single-precision scalars differ in kind from every other fp32 test: the
# clipped and then saturated schedule, mu four decades from the drivers', and
# thr = lambda/mu = 1e33, still finite in single.
F32_R16_IN_SUITE = ("sat_clip", "mu_small", "lam_huge")
F32_CELLS = tuple((g, 4) for g in F32_ADMITTED[4]) + tuple((g, 16) for g in F32_R16_IN_SUITE)
F32_MIN_AT_R4 = 8


# ---------------------------------------------------------------------------
# the nonconvex solver: one deviation from sweep_cases.NCVX_PARAMS per row
# ---------------------------------------------------------------------------
NCVX_ITERS = 8
NCVX_R = 5
NCVX_ROWS = {
    "theta_eq_p": dict(theta=0.5),                 # exponent theta - p = 0: unit weights
    "expo_neg": dict(theta=0.25, p=0.75),          # negative exponent
    "p1_theta1": dict(p=1.0, theta=1.0),
    "gammaA_zero": dict(gamma_A=0.0),              # no shrink of A
    # gamma_A = 0.05 shrinks two of the 25 columns of the unfolded A to zero on
    # the unmasked inputs (the next Gram is then singular and B, C answer a
    # 1e-14 perturbation with 8e-8 and 1e-5); 0.04 keeps at least 2 nonzeros in
    # every column (17 under the mask) and 58 % of A
    "gammaA_big": dict(gamma_A=0.04),
    "eps_tiny": dict(epsilon=1e-12),
    "rho_quarter": dict(rho=0.25),
    "rho8": dict(rho=8.0),
    "lam_zero": dict(lam=0.0),                     # O keeps every residue
    "lam_huge": dict(lam=1e30),                    # O identically zero
}
NCVX_IDS = tuple(NCVX_ROWS)


def ncvx_args(row):
    return sc.ncvx_args(dict(NCVX_ROWS[row], maxIter=NCVX_ITERS, tol=0.0))


def _quiet(s):
    pass


def ncvx_solve(row, X=None, A0=None, obs=None, r=NCVX_R):
    """The (masked) nonconvex oracle on the sweep inputs: dict(A, B, C, O, errHist, k)."""
    import masked_ncvx_cases as mnc
    import masked_ncvx_oracle as mno
    import tritd_oracle as orc
    c = sc.e_active_case(r)
    X = c["D"] if X is None else X
    A0 = c["A0"] if A0 is None else A0
    if obs is None:
        t = orc.triple_decomp_ADMM_ncvx(X, r, *ncvx_args(row), A0, c["B0"], c["C0"], printer=_quiet)
    else:
        t = mno.triple_decomp_ncvx_masked(X, obs, r, *ncvx_args(row), A0, c["B0"], c["C0"],
                                          printer=_quiet)
    return mnc.as_ref(t)


@functools.lru_cache(maxsize=None)
def ncvx_ref(row, masked=False):
    return ncvx_solve(row, obs=observed(NCVX_R) if masked else None)


# ---------------------------------------------------------------------------
# the session's own switch to dense-E storage (solver.cpp Session::maybe_dense_e)
# ---------------------------------------------------------------------------
# After iterations 8 and 24 the session divides the dense tiles counted since
# the last check by launches x tiles per launch and switches at 0.5 or more.
# Session::counters reports tiles per launch as Ntm / 256 with Ntm =
# tiles4 ntt 256 (csrc/common.h make_geom): the ij-tiles n1p/16 * n2 rounded up
# to K5's workgroups of four, times the t-tiles n3p/16, so the padding tiles
# of the last workgroup are in the denominator (r = 5: 60 x 3 = 180 against the
# 171 tiles that exist).
def tiles_per_launch(shape):
    n1, n2, n3 = shape
    tiles = (n1 + 15) // 16 * n2
    return (tiles + 3) // 4 * 4 * ((n3 + 15) // 16)


def counter_share(E):
    """Dense tiles of one launch over tiles per launch, as maybe_dense_e forms it."""
    return float(np.sum(kc.tile_counts(E) > kc.CE_CAP)) / tiles_per_launch(np.shape(E))


def window_shares(shares):
    """(mean over iterations 1-8, mean over 9-24) of per-iteration shares."""
    return float(np.mean(shares[:8])), float(np.mean(shares[8:24]))


SWITCH_R = 5
# regime: None for the sweep's own options; n iterations, run in `steps`
SWITCH24 = dict(regime=None, n=26, steps=(10, 16), share8_max=0.40, share24_min=0.58)
SWITCH8 = dict(regime="lam_zero", n=12, steps=(12,))
NO_SWITCH = dict(regime="rho1", n=26, steps=(26,), share_max=0.01)


def switch_case(regime, n):
    """Inputs of a dense-E switch case at SWITCH_R: the sweep's own options
    (regime None) or a regime's, n iterations, maxIter = n + 1 so that the
    profiling iteration after the run is inside maxIter."""
    c = sc.e_active_case(SWITCH_R) if regime is None else case(regime, SWITCH_R)
    c["opts"] = dict(c["opts"], maxIter=n + 1)
    return c


@functools.lru_cache(maxsize=None)
def switch_ref(regime, n):
    import tritd_oracle as orc
    c = switch_case(regime, n)
    return sc.as_ref(orc.triple_decomp_ADMM(c["D"], c["r"], dict(c["opts"], maxIter=n), c["A0"],
                                            c["B0"], c["C0"]))


@functools.lru_cache(maxsize=None)
def switch_shares(regime, n):
    c = switch_case(regime, n)
    return tuple(counter_share(E) for E in e_per_iteration(c, n))
