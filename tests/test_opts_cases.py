"""CPU: the option ladder (tests/opts_cases.py) is well posed, from the
references alone.

tests/test_gpu_opts_ladder.py compares at the suite's tolerances (L, O, E
1e-9; A, B, C 1e-8; fp32 2e-5); a miss there must mean a wrong scalar or
kernel, not an ill-conditioned regime.  For every cell (regime, rank, form)
that module runs:

  * the reference is finite and runs the regime's iteration count, and no
    relative change of errHist comes within 10x of opts.tol (the stop test
    is never a coin flip);
  * the schedule property the regime is named for really occurs within the
    run (mu_k recomputed here);
  * E is as declared: all zero (lam_huge), nonzero at every observed entry
    (lam_zero), some tile going from a dense tile back to a compact slot
    (rho1_lam1), active after 3 iterations (the rest);
  * the reference moves by at most 1e-11 on L, O, E and 1e-10 on A, B, C when
    D is perturbed by relative 1e-14 (a hundredth of the GPU tolerances).
    Measured: at most 1.6e-12 on L, O, E (rho_dec, r = 11) and 1.2e-12 on
    A, B, C (rho_dec, r = 5); no fp64 cell is dropped;
  * fp32: the class-single restatement moves by at most a quarter of the fp32
    tolerance under input rounding for every cell of opts_cases.F32_CELLS
    (all 13 regimes at r = 4, three at r = 16; opts_cases.F32_ADMITTED records
    the measured response of all 26 cells and why six stable r = 16 cells are
    not run);
  * the rows of the nonconvex table: finite, 8 iterations, the same response
    bound on A, B, C and O, and every column of the unfolded A keeps a nonzero
    under the strongest shrink;
  * the inputs of the unforced dense-E switch have the dense-tile shares the
    GPU tests rely on, with the denominator Session::counters reports.
"""
import numpy as np
import pytest

import k5_step_bits_cases as kc
import opts_cases as oc
import sweep_cases as sc
from conftest import rel

import masked_oracle as mo
import tritd_oracle as orc

U32 = 2.0 ** -24
STOP_MARGIN = 10.0

# every fp64 cell of the GPU module: (regime, rank, form)
CELLS = ([(g, r, "cp") for r in oc.RANKS for g in oc.IDS]
         + [(g, oc.R_FORMS, "masked") for g in oc.IDS]
         + [(g, oc.R_DEVICE_SET, "cp") for g in oc.SUBSET]
         + [(g, oc.R_FORMS, "qi") for g in oc.SUBSET])


def _ref(regime, r, form, n=None):
    if form == "masked":
        return oc.masked_ref(regime, r, n)
    return oc.ref(regime, r, form, n)


def _is_step(ratio, rho):
    return abs(ratio - rho) <= 1e-12 * rho


@pytest.mark.parametrize("regime", oc.IDS)
def test_schedule_property_occurs_within_the_run(regime):
    """mu_1 .. mu_iters as Session::scalars reads them (mu_[k-1] at iteration k)."""
    over, n = oc.REGIMES[regime]
    mu = oc.schedule(regime)[:n]
    mu0, rho = over.get("mu", 1e-3), over.get("rho", 1.25)
    ratio = mu[1:] / mu[:-1]
    short = [x for x in ratio if 1.0 < x and not _is_step(x, rho)]
    print(regime, mu, ratio)
    assert mu[0] == mu0
    if regime in oc.SATURATING:
        assert mu[-1] == mu0 * 1e6 and ratio[-1] == 1.0  # reached, and held for a step
        first = int(np.argmax(mu == mu0 * 1e6)) + 1      # the first saturated iteration
        assert first == {"sat_fast": 2, "sat_mid": 7, "sat_clip": 11}[regime]
        if regime == "sat_clip":
            assert len(short) == 1 and 1.0 < short[0] < rho
            assert first < n - 1                         # cprev = 1 follows the short step
        else:
            assert not short
    elif rho == 1.0:
        assert np.all(mu == mu0)                         # cprev = 1, invL_next = invL
    else:
        assert all(_is_step(x, rho) for x in ratio)      # the clip never acts
        assert mu[-1] < mu0 * 1e6
    if regime == "rho_dec":
        assert abs(mu[-2] / mu[-1] - 1.25) <= 1e-12      # cprev
    if regime == "mu1_rho1":
        assert mu0 == 1.0
    if regime == "lam_huge":                             # thr = lambda / mu is finite in single
        assert np.isfinite(np.float32(1e30 / mu.min()))


@pytest.mark.parametrize("regime, r, form", CELLS)
def test_cell_is_finite_declared_and_stable(regime, r, form):
    assert (regime, r, form) not in oc.DROPPED64
    masked = form == "masked"
    model = "cp" if masked else form
    c = oc.case(regime, r, model=model)
    obs = oc.observed(r) if masked else np.ones(c["D"].shape, dtype=bool)
    a = _ref(regime, r, form)
    # finite, every iteration run, the stop test far from firing
    for key in ("A", "B", "C", "O", "E", "errHist"):
        assert np.isfinite(a[key]).all(), key
    assert a["k"] == oc.iters(regime) == len(a["errHist"])
    eh = a["errHist"]
    change = np.abs(np.diff(eh)) / eh[:-1]
    assert change.min() >= STOP_MARGIN * c["opts"]["tol"], change.min()
    # E as declared
    E = a["E"]
    if regime == "lam_huge":
        assert not np.any(E)
    elif regime == "lam_zero":
        assert np.all(E[obs] != 0)
    else:
        assert np.count_nonzero(_ref(regime, r, form, 3)["E"]) > 0
    if regime == "rho1_lam1":
        cnt = [kc.tile_counts(x) for x in oc.e_per_iteration(c, oc.iters(regime), obs if masked else None)]
        back = [int(np.sum((p > kc.CE_CAP) & (q >= 1) & (q <= kc.CE_CAP))) for p, q in zip(cnt, cnt[1:])]
        print("  tiles returning from dense to a compact slot, per iteration:", back)
        assert max(back) >= 1
    # response to a 1e-14 relative perturbation of D
    Dp = sc.perturbed(c["D"], 1e-14, np.random.default_rng(1))
    if masked:
        b = mo.triple_decomp_ADMM_masked(Dp, obs, r, c["opts"], c["A0"], c["B0"], c["C0"])
    else:
        b = orc.triple_decomp_ADMM(Dp, r, c["opts"], c["A0"], c["B0"], c["C0"])
    b = sc.as_ref(b)
    assert b["k"] == a["k"]
    loe = max(rel(orc.triple_product(b["A"], b["B"], b["C"], model),
                  orc.triple_product(a["A"], a["B"], a["C"], model)), rel(b["O"], a["O"]), rel(b["E"], E))
    abc = max(rel(b[key], a[key]) for key in "ABC")
    print("  %s r=%d %s nnz(E)=%.3f response L,O,E %.1e  A,B,C %.1e" % (regime, r, form, sc.nnz_share(E),
                                                                       loe, abc))
    assert loe <= oc.RESPONSE_LOE and abc <= oc.RESPONSE_ABC


def test_at_most_two_fp64_cells_are_dropped():
    assert len(oc.DROPPED64) <= 2


# ---------------------------------------------------------------------------
# fp32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("regime, r", oc.F32_CELLS)
def test_fp32_cell_is_stable_under_input_rounding(regime, r):
    """The rule of tests/test_sweep_cases.py at a quarter of test_gpu_f32.TOL,
    for every cell the GPU module runs (opts_cases.F32_ADMITTED lists the
    measured responses, those of the cells left out included).  An r = 16 cell
    takes about a minute: four solves of the restatement at R = 256."""
    from test_gpu_f32 import TOL
    assert oc.F32_RESPONSE_MAX == TOL / 4
    mod, lib = sc.cref_lib()
    c = oc.case(regime, r, np.float32)
    base = oc.c_ref32(regime, r)
    for key in ("A", "B", "C", "O", "E", "errHist"):
        assert np.isfinite(base[key]).all(), key
    assert base["k"] == oc.iters(regime)
    assert bool(np.any(base["E"])) == (regime != "lam_huge")
    L0 = orc.triple_product(base["A"], base["B"], base["C"])
    worst, same_k = 0.0, True
    for seed in (1, 2, 3):
        rng = np.random.default_rng(1000 * r + seed)
        D = sc.perturbed(c["D"], U32, rng)
        A0 = sc.perturbed(c["A0"], U32, rng)
        p = mod.admm(lib, D, c["r"], c["opts"], A0, c["B0"], c["C0"])
        same_k = same_k and p[6] == base["k"]
        worst = max(worst, rel(orc.triple_product(p[0], p[1], p[2]), L0),
                    rel(p[3].astype(np.float64), base["O"].astype(np.float64)),
                    rel(p[5].astype(np.float64), base["E"].astype(np.float64)))
    print("%s r=%d fp32 perturbation response %.2e" % (regime, r, worst))
    assert same_k and worst <= oc.F32_RESPONSE_MAX


def test_enough_fp32_regimes_remain():
    assert len(oc.F32_ADMITTED[4]) >= oc.F32_MIN_AT_R4
    assert all(set(v) <= set(oc.IDS) for v in oc.F32_ADMITTED.values())
    assert set(oc.F32_CELLS) <= {(g, r) for r, v in oc.F32_ADMITTED.items() for g in v}


# ---------------------------------------------------------------------------
# the nonconvex solver
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("row", oc.NCVX_IDS)
def test_ncvx_row_is_finite_and_stable(row, masked):
    over = set(oc.NCVX_ROWS[row])  # one deviation per row: one option, or the exponent's pair
    assert len(over) == 1 or over == {"theta", "p"}
    a = oc.ncvx_ref(row, masked)
    for key in ("A", "B", "C", "O", "errHist"):
        assert np.isfinite(a[key]).all(), key
    assert a["k"] == oc.NCVX_ITERS == len(a["errHist"])
    assert bool(np.any(a["O"])) == (row != "lam_huge")
    A1 = a["A"].reshape(a["A"].shape[0], -1, order="F")
    per_column = np.count_nonzero(A1, axis=0)
    assert per_column.min() >= 1, "a column of A was shrunk to zero: the next Gram is singular"
    c = sc.e_active_case(oc.NCVX_R)
    b = oc.ncvx_solve(row, X=sc.perturbed(c["D"], 1e-14, np.random.default_rng(1)),
                      obs=oc.observed(oc.NCVX_R) if masked else None)
    moved = {key: rel(b[key], a[key]) for key in ("A", "B", "C", "O")}
    print("  ncvx %s masked=%d nnz(O)=%.3f nnz(A)=%.3f min column nnz %d response %s" % (
        row, masked, sc.nnz_share(a["O"]), sc.nnz_share(a["A"]), per_column.min(),
        {k: "%.1e" % v for k, v in moved.items()}))
    assert b["k"] == a["k"]
    assert moved["O"] <= oc.RESPONSE_LOE and max(moved[key] for key in "ABC") <= oc.RESPONSE_ABC


def test_ncvx_exponents_are_what_the_rows_say():
    prm = {row: dict(sc.NCVX_PARAMS, **over) for row, over in oc.NCVX_ROWS.items()}
    assert sc.NCVX_PARAMS["theta"] - sc.NCVX_PARAMS["p"] > 0  # every older test: a positive exponent
    assert prm["theta_eq_p"]["theta"] - prm["theta_eq_p"]["p"] == 0.0
    assert prm["expo_neg"]["theta"] - prm["expo_neg"]["p"] == -0.5
    assert prm["p1_theta1"]["theta"] == prm["p1_theta1"]["p"] == 1.0
    # the strongest shrink really removes entries of A, the weakest none
    assert sc.nnz_share(oc.ncvx_ref("gammaA_big")["A"]) < 0.7
    assert sc.nnz_share(oc.ncvx_ref("gammaA_zero")["A"]) == 1.0


# ---------------------------------------------------------------------------
# the unforced dense-E switch
# ---------------------------------------------------------------------------
def test_tiles_per_launch_counts_the_padding_tiles_of_the_last_workgroup():
    shape = sc.e_active_shape(oc.SWITCH_R)
    assert shape == (37, 19, 34)
    assert oc.tiles_per_launch(shape) == 180                     # 3 * 19 = 57 -> 60 ij-tiles, 3 t-tiles
    assert kc.tile_counts(np.zeros(shape)).size == 171           # of which 171 exist


@pytest.mark.parametrize("cfg", [oc.SWITCH24, oc.SWITCH8, oc.NO_SWITCH],
                         ids=["switch_at_24", "switch_at_8", "no_switch"])
def test_dense_e_switch_inputs(cfg):
    """Dense-tile shares of the oracle's E over the two windows maybe_dense_e
    sums (iterations 1-8 and 9-24), against its threshold of 0.5."""
    n = cfg["n"]
    a = oc.switch_ref(cfg["regime"], n)
    c = oc.switch_case(cfg["regime"], n)
    assert a["k"] == n and c["opts"]["maxIter"] == n + 1 and sum(cfg["steps"]) == n
    change = np.abs(np.diff(a["errHist"])) / a["errHist"][:-1]
    assert change.min() >= STOP_MARGIN * c["opts"]["tol"], change.min()
    shares = oc.switch_shares(cfg["regime"], n)
    first, second = oc.window_shares(shares + (0.0,) * 24)
    print("  dense share, iterations 1-8: %.3f, 9-24: %.3f; per iteration %s" % (
        first, second, " ".join("%.2f" % s for s in shares)))
    if cfg is oc.SWITCH24:
        assert first <= cfg["share8_max"] < 0.5 and second >= cfg["share24_min"] > 0.5
        assert cfg["steps"][0] > 8 and cfg["steps"][0] < 24      # the first step passes the check at 8 only
    elif cfg is oc.SWITCH8:
        assert first > 0.5 and np.all(a["E"] != 0) and n > 8
    else:
        assert max(shares) < cfg["share_max"] and n > 24
        assert np.any(a["E"])


def test_switch_at_24_reference_is_stable():
    """The 26-iteration reference of the switch-at-24 case under the 1e-14 perturbation."""
    n = oc.SWITCH24["n"]
    for regime in (None, "rho1"):
        c = oc.switch_case(regime, n)
        a = oc.switch_ref(regime, n)
        b = sc.as_ref(orc.triple_decomp_ADMM(sc.perturbed(c["D"], 1e-14, np.random.default_rng(1)), c["r"],
                                             dict(c["opts"], maxIter=n), c["A0"], c["B0"], c["C0"]))
        loe = max(rel(orc.triple_product(b["A"], b["B"], b["C"]), orc.triple_product(a["A"], a["B"], a["C"])),
                  rel(b["O"], a["O"]), rel(b["E"], a["E"]))
        abc = max(rel(b[key], a[key]) for key in "ABC")
        print("  %s, %d iterations: response L,O,E %.1e  A,B,C %.1e" % (regime, n, loe, abc))
        assert loe <= oc.RESPONSE_LOE and abc <= oc.RESPONSE_ABC
