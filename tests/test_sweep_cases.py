"""CPU: the E-active rank-sweep inputs (tests/sweep_cases.py) are well posed.

The GPU sweeps (tests/test_gpu_rank_sweep.py, test_gpu_f32.py, the ALS / Qi /
nonconvex modules) compare at tight tolerances; a miss there must mean a
kernel fault, not an ill-conditioned case.  For every rank r = 1..16, and for
the tall case (97 x 83 x 85 at r = 7, past the one-launch apply + Gram):

  * E is active and mixed: nnz(E) >= 0.5 % after 3 iterations, within
    10..70 % after 10; at least 10 % of the 16 x 16 (i, t) tiles hold 1..28
    nonzeros (compact slots) and at least 10 % hold more (dense tiles).
  * fp64: the numpy oracle and the C restatement (two independent summation
    orders) agree to <= 1e-11 on L, O, E, A, B, C and errHist — a hundredth of
    the GPU tolerance of 1e-9.
  * fp32: the class-single C restatement moves by <= 4e-6 (a fifth of the
    fp32 GPU tolerance 2e-5) on L, O, E when D and A0 are perturbed by
    relative 2^-24 U(-1, 1), three seeds.

And for the ALS, Qi-ADMM and nonconvex cases: the oracle moves by < 1e-11 when
its inputs are perturbed at relative 2^-52.
"""
import numpy as np
import pytest

import sweep_cases as sc
from conftest import rel

import tritd_oracle as orc

U32 = 2.0 ** -24
U64 = 2.0 ** -52


CASES = sc.RANKS + (sc.TALL,)


def test_tall_case_is_past_the_one_launch_threshold():
    """rows * RP^2 > 327 680 for each of A^ (n1p rows), B^ (n2), C^ (n3p) at RP = 64."""
    n1, n2, n3 = sc.case_shape(sc.TALL)
    RP = -(-sc.TALL_RANK ** 2 // 16) * 16
    assert RP == 64
    assert min(-(-n1 // 16) * 16, n2, -(-n3 // 16) * 16) * RP * RP > 327680


@pytest.mark.parametrize("r", CASES)
def test_e_is_active_and_mixed(r):
    shape = sc.case_shape(r)
    assert all(n % 16 for n in shape) and shape[0] > 16 and shape[2] > 16
    nnz3 = sc.nnz_share(sc.oracle_ref(r, iters=3)["E"])
    E = sc.oracle_ref(r)["E"]
    nnz = sc.nnz_share(E)
    compact, dense = sc.tile_shares(E)
    print("r=%s nnz3=%.4f nnz10=%.4f compact=%.3f dense=%.3f" % (r, nnz3, nnz, compact, dense))
    assert nnz3 >= sc.NNZ3_MIN
    assert sc.NNZ_BAND[0] <= nnz <= sc.NNZ_BAND[1]
    assert compact >= sc.TILE_SHARE_MIN and dense >= sc.TILE_SHARE_MIN


@pytest.mark.parametrize("r", CASES)
def test_fp64_oracle_and_c_restatement_agree(r):
    a, b = sc.oracle_ref(r), sc.c_ref(r, False)
    assert a["k"] == b["k"] == sc.ITERS
    worst = {"L": rel(orc.triple_product(b["A"], b["B"], b["C"]),
                      orc.triple_product(a["A"], a["B"], a["C"]))}
    for key in ("O", "E", "A", "B", "C", "errHist"):
        worst[key] = rel(b[key], a[key])
    print("r=%s" % r, {k: "%.1e" % v for k, v in worst.items()})
    assert max(worst.values()) <= 1e-11, worst


@pytest.mark.parametrize("r", CASES)
def test_fp32_restatement_is_stable_under_input_rounding(r):
    mod, lib = sc.cref_lib()
    c = sc.e_active_case(r, np.float32)
    base = sc.c_ref(r, True)
    L0 = orc.triple_product(base["A"], base["B"], base["C"])
    assert np.any(base["E"])
    worst = 0.0
    for seed in (1, 2, 3):
        rng = np.random.default_rng(1000 * (0 if r == sc.TALL else r) + seed)
        D = sc.perturbed(c["D"], U32, rng)
        A0 = sc.perturbed(c["A0"], U32, rng)
        p = mod.admm(lib, D, c["r"], c["opts"], A0, c["B0"], c["C0"])
        assert p[6] == base["k"]
        worst = max(worst, rel(orc.triple_product(p[0], p[1], p[2]), L0),
                    rel(p[3].astype(np.float64), base["O"].astype(np.float64)),
                    rel(p[5].astype(np.float64), base["E"].astype(np.float64)))
    print("r=%s fp32 perturbation response %.2e" % (r, worst))
    assert worst <= 4e-6


def _moved(a, b, keys):
    return max(rel(np.asarray(b[i], np.float64), np.asarray(a[i], np.float64)) for i in keys)


@pytest.mark.parametrize("r", [4, 6, 7])
def test_als_and_ncvx_oracles_are_stable_under_input_rounding(r):
    c = sc.e_active_case(r)
    rng = np.random.default_rng(r)
    X, A0 = sc.perturbed(c["D"], U64, rng), sc.perturbed(c["A0"], U64, rng)
    als = _moved(sc.oracle_als_ref(r), sc.oracle_als(r, X, A0), range(4))       # A, B, C, errHist
    ncv = _moved(sc.oracle_ncvx_ref(r), sc.oracle_ncvx(r, X, A0), range(5))     # A, B, C, O, errHist
    print("r=%d ALS moved %.1e, nonconvex moved %.1e" % (r, als, ncv))
    assert als < 1e-11 and ncv < 1e-11


@pytest.mark.parametrize("r", [1, 4, 5, 6, 7])
def test_qi_case_is_active_and_stable(r):
    c = sc.e_active_case(r, model="qi")
    assert c["opts"]["model"] == "qi"
    base = sc.oracle_ref(r, model="qi")
    nnz = sc.nnz_share(base["E"])
    assert sc.NNZ_BAND[0] <= nnz <= sc.NNZ_BAND[1]
    rng = np.random.default_rng(r)
    p = sc.as_ref(orc.triple_decomp_ADMM(sc.perturbed(c["D"], U64, rng), r, c["opts"],
                                         sc.perturbed(c["A0"], U64, rng), c["B0"], c["C0"]))
    moved = max(rel(p[k], base[k]) for k in ("A", "B", "C", "O", "E", "errHist"))
    print("r=%d qi nnz=%.3f moved %.1e" % (r, nnz, moved))
    assert moved < 1e-11
