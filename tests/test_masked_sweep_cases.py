"""CPU: the masked rank-sweep inputs (tests/masked_sweep_cases.py) are what
tests/test_gpu_masked_rank_sweep.py takes them for.  Every condition is one the
masked oracle alone must satisfy, so a miss on the GPU means a kernel fault,
not an ill-conditioned or dormant case.

  * Admission rule of tests/golden/make_masked_golden.py: the oracle rerun with
    D, A0, B0 and C0 perturbed by 1e-15 relative (three seeds) stops at the
    same k and moves L, O, E, A, B, C and errHist by at least 100x less than
    their tolerances.  Measured over the 24 cases: L, O, E <= 1.5e-13; A, B, C
    <= 6.4e-14; errHist <= 7.1e-6 of its gate.
  * E is active: nnz(E) / nnz(observed) within 4..75 % after 10 iterations
    (measured 5.0 % at cp r = 2 to 70.9 % at qi r = 7) and >= 0.3 % after 3
    (measured 0.4 % at cp r = 16).
  * Both storage forms: >= 8 % of the 16 x 16 (i, t) tiles hold 1..28 nonzeros
    (compact slots) and >= 8 % hold more (dense tiles), except for the three
    cases listed as compact-only (nnz about 5 %, no dense tile).  Measured over
    the other 21: compact 12.7..88.4 %, dense 8.1..86.2 %.
  * The mask: 14..18 % missing, the three blocks, no row, fibre or slice
    without an observed entry.
  * The hidden-shard masks (cp r = 3, 6, 11) pass the same rule and mix both
    forms (dense share 24, 45, 62 %).
  * With an all-true mask the masked oracle is the unmasked oracle, bitwise.
"""
import numpy as np
import pytest

import masked_oracle as mo
import masked_sweep_cases as ms
import sweep_cases as sc

IDS = [ms.case_id(c) for c in ms.CASES]
HIDDEN = [("cp", r) for r in ms.HIDDEN_RANKS]


def assert_admitted(d, label):
    print(label, " ".join("%s=%.1e" % kv for kv in d.items()))
    assert d["k"] == 0.0
    for key in ("L", "O", "E"):
        assert ms.MARGIN * d[key] <= ms.TOL_LOE, (key, d[key])
    assert ms.MARGIN * d["ABC"] <= ms.TOL_ABC, d["ABC"]
    assert ms.MARGIN * d["errHist_gate"] <= 1.0, d["errHist_gate"]


def test_the_cases_and_the_schedule_ranks():
    assert ms.CASES == tuple(("cp", r) for r in range(1, 17)) + tuple(("qi", r) for r in range(1, 9))
    assert ms.ITERS == 10

    def padded(r):  # Geom's padded rank (csrc/common.h)
        return next(p for p in (16, 32, 48, 64, 128, 256) if r * r <= p)

    assert [padded(r) for r in ms.SCHEDULE_RANKS] == [16, 32, 48, 64, 128, 256]
    assert ms.NARROW == tuple(r for r in ms.SCHEDULE_RANKS if padded(r) <= 64)
    assert {padded(r) for r in range(1, 9)} == {16, 32, 48, 64}  # the Qi cases


@pytest.mark.parametrize("case", ms.CASES, ids=IDS)
def test_inputs(case):
    model, r = case
    c, base = ms.inputs(case), sc.e_active_case(r, model=model)
    assert c["D"].shape == (35 + r % 3, 19 + r % 5, 33 + r % 4) and c["D"].flags.f_contiguous
    assert c["opts"]["maxIter"] == ms.ITERS and c["opts"].get("model", "cp") == model
    assert c["opts"]["lambda"] == 2e-3 * float(np.std(c["D"]))
    assert c["opts"] == base["opts"]
    for key in ("D", "A0", "B0", "C0"):
        np.testing.assert_array_equal(c[key], base[key])


@pytest.mark.parametrize("case", ms.CASES, ids=IDS)
def test_mask_structure(case):
    W = ms.mask(case)
    n1, n2, n3 = shape = sc.e_active_shape(case[1])
    assert W.shape == shape and W.dtype == bool and W.flags.f_contiguous
    missing = 1.0 - W.mean()
    print(ms.case_id(case), "missing %.3f" % missing)
    assert ms.MISSING_BAND[0] <= missing <= ms.MISSING_BAND[1]
    assert not W[:16, 1, 16:32].any()          # a whole tile missing
    assert not W[32:, 2, :16].any() and 0 < n1 - 32 < 16  # the real rows of a ragged edge tile
    assert W[:16, 3, :16].all()                 # a fully observed tile
    assert W.any(axis=(1, 2)).all() and W.any(axis=(0, 2)).all() and W.any(axis=(0, 1)).all()
    # outside the three blocks: the random draw
    rnd = np.random.default_rng([case[1], 7]).random(shape) >= 0.15
    same = W == rnd
    same[:16, 1, 16:32] = same[32:, 2, :16] = same[:16, 3, :16] = True
    assert same.all()


@pytest.mark.parametrize("case", ms.CASES, ids=IDS)
def test_admission_rule(case):
    ref = ms.reference(case)
    assert ref["k"] == ms.ITERS and len(ref["errHist"]) == ms.ITERS
    assert_admitted(ms.drifts(ms.inputs(case), ref), ms.case_id(case))


@pytest.mark.parametrize("case", ms.CASES, ids=IDS)
def test_e_is_active_and_zero_where_unobserved(case):
    W, ref = ms.mask(case), ms.reference(case)
    nnz3 = ms.nnz_of_observed(ms.reference(case, 3)["E"], W)
    nnz = ms.nnz_of_observed(ref["E"], W)
    print(ms.case_id(case), "nnz3=%.4f nnz10=%.4f" % (nnz3, nnz))
    assert nnz3 >= ms.NNZ3_MIN
    assert ms.NNZ_BAND[0] <= nnz <= ms.NNZ_BAND[1]
    assert not ref["O"][~W].any() and not ref["E"][~W].any()


@pytest.mark.parametrize("case", ms.CASES, ids=IDS)
def test_storage_forms(case):
    compact, dense = sc.tile_shares(ms.reference(case)["E"])
    print(ms.case_id(case), "compact=%.3f dense=%.3f" % (compact, dense))
    assert compact >= ms.TILE_SHARE_MIN
    if case in ms.COMPACT_ONLY:
        assert dense < ms.TILE_SHARE_MIN  # (else the case belongs with the mixed ones)
    else:
        assert dense >= ms.TILE_SHARE_MIN


def test_the_schedule_ranks_mix_both_forms():
    for case in [("cp", r) for r in ms.SCHEDULE_RANKS] + [("qi", 6)] + HIDDEN:
        assert case in ms.CASES and case not in ms.COMPACT_ONLY, case
    assert set(ms.COMPACT_ONLY) == {("cp", 2), ("cp", 4), ("qi", 3)}


@pytest.mark.parametrize("case", HIDDEN, ids=[ms.case_id(c) for c in HIDDEN])
def test_hidden_shard_masks(case):
    W, H = ms.mask(case), ms.hidden_shard_mask(case)
    rows = W.shape[0] // 3
    assert not H[:rows].any() and np.array_equal(H[rows:], W[rows:]) and H.flags.f_contiguous
    assert H[rows:].any(axis=(1, 2)).all() and H.any(axis=(0, 2)).all() and H.any(axis=(0, 1)).all()
    ref = ms.hidden_reference(case)
    assert ref["k"] == ms.ITERS and np.isfinite(ref["errHist"]).all()
    assert not ref["O"][~H].any() and not ref["E"][~H].any()
    assert_admitted(ms.drifts(ms.inputs(case, H), ref), ms.case_id(case) + " hidden")
    compact, dense = sc.tile_shares(ref["E"])
    print(ms.case_id(case), "hidden compact=%.3f dense=%.3f" % (compact, dense))
    assert compact >= ms.TILE_SHARE_MIN and dense >= ms.TILE_SHARE_MIN


@pytest.mark.parametrize("r", [6, 10])
def test_all_true_mask_is_the_unmasked_oracle_bitwise(r):
    c, ref = sc.e_active_case(r), sc.oracle_ref(r)
    got = sc.as_ref(mo.triple_decomp_ADMM_masked(c["D"], np.ones(c["D"].shape, dtype=bool), r,
                                                 c["opts"], c["A0"], c["B0"], c["C0"]))
    assert got["k"] == ref["k"]
    for key in ("A", "B", "C", "O", "errHist", "E"):
        np.testing.assert_array_equal(got[key], ref[key])
