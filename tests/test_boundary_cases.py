"""CPU: the inputs of tests/test_gpu_session_boundary.py (tests/boundary_cases.py)
are what the GPU module takes them for.

  * rre_parts references: for X1 = Lstar and X2 (independent normal) every
    case, after 10 iterations and before any, has |L_ref - X| >= 0.1 |L_ref|,
    so the derived tolerance of num stays at or below 3e-12 there; X3 is in
    the near-converged regime (|L_ref - X3| between 1e-7 and 1e-6 of |L_ref|),
    where that tolerance is between 1e-7 and 1e-5 — far below the O(1) change
    a misread element makes, as the last test shows.
  * padded(): the shard's elements sit at off + i + ld (j + n2 t) and every
    other element of the buffer is NaN.
  * the degenerate and the sub-range problems are well conditioned: the numpy
    oracle and the C restatement agree to a hundredth of the GPU tolerance
    they are compared at.
  * a restatement that sums one padded row, skips the last t, or reads X with
    the wrong stride misses the tolerances by orders of magnitude.
"""
import numpy as np
import pytest

import boundary_cases as bc
import sweep_cases as sc
from conftest import rel

import tritd_oracle as orc

IDS = [bc.case_id(c) for c in bc.CASES]


def test_case_list():
    padded_rank = {4: 16, 5: 32, 6: 48, 8: 64, 11: 128, 16: 256}
    assert [padded_rank[r] for r in bc.RANKS] == [16, 32, 48, 64, 128, 256]
    for shape, _ in bc.DEGENERATE:
        assert 1 in shape
    for case in bc.CASES:
        c = bc.inputs(case)
        assert c["opts"]["maxIter"] == bc.ITERS == 10 and c["opts"]["tol"] == 1e-5
        assert c["D"].dtype == (np.float32 if case[0] == "f32" else np.float64)
        assert c["D"].flags.f_contiguous and c["Lstar"].shape == c["D"].shape
        assert c["Lstar"].dtype == np.float64
    for r in bc.SUB_RANKS:
        n1 = sc.e_active_shape(r)[0]
        i0, i1 = bc.sub_range(n1)
        assert (i0, i1) == (5, n1 - 4) and (i1 - i0) % 16 and i1 - i0 > 16  # two local tiles, ragged


@pytest.mark.parametrize("fresh", [False, True], ids=["iterated", "fresh"])
@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_rre_tensors_are_far_or_near_as_stated(case, fresh):
    L = bc.reference_product(case, fresh)
    nL = float(np.linalg.norm(L.ravel()))
    X1, X2, X3 = bc.rre_tensors(case, fresh)
    dist = [float(np.linalg.norm((L - X.astype(np.float64)).ravel())) / nL for X in (X1, X2, X3)]
    tols = [bc.rre_reference(L, X)[2] for X in (X1, X2, X3)]
    print(bc.case_id(case), "fresh" if fresh else "iterated",
          "|L-X|/|L| = %.3g %.3g %.3g, rtol(num) = %.2g %.2g %.2g" % tuple(dist + tols))
    assert dist[0] >= bc.FAR and dist[1] >= bc.FAR
    assert tols[0] <= 3e-12 and tols[1] <= 3e-12
    assert 1e-7 <= dist[2] <= 1e-6 and 1e-7 <= tols[2] <= 1e-5
    dt = np.float32 if case[0] == "f32" else np.float64
    assert all(X.dtype == dt and X.flags.f_contiguous for X in (X1, X2, X3))


@pytest.mark.parametrize("form", list(bc.FORMS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_padded_layout(form, dtype):
    X = np.asfortranarray(np.arange(1, 1 + 5 * 3 * 4, dtype=dtype).reshape((5, 3, 4), order="F"))
    buf, ld, off = bc.padded(X, form)
    extra, o = bc.FORMS[form]
    assert (ld, off) == (5 + extra, o) and buf.dtype == dtype and buf.flags.f_contiguous
    flat = buf.ravel(order="K")
    assert flat.size == ld * 3 * 4
    seen = np.zeros(flat.size, bool)
    for t in range(4):
        for j in range(3):
            for i in range(5):
                e = off + i + ld * (j + 3 * t)
                assert flat[e] == X[i, j, t]
                seen[e] = True
    assert np.all(np.isnan(flat[~seen])) and np.count_nonzero(~seen) == extra * 3 * 4
    if form == "offset":
        assert off % 2 == 1  # the pointer the session gets is only element-aligned


@pytest.mark.parametrize("q", range(len(bc.DEGENERATE)))
def test_degenerate_cases_are_active_and_well_conditioned(q):
    """test_gpu_parity compares these shapes at 1e-8 (errHist rtol 1e-7)."""
    mod, lib = sc.cref_lib()
    case = ("deg", q)
    c = bc.inputs(case)
    a = bc.reference(case)
    b = sc.as_ref(mod.admm(lib, c["D"], c["r"], c["opts"], c["A0"], c["B0"], c["C0"]))
    assert a["k"] == b["k"] == bc.ITERS
    nnz = sc.nnz_share(a["E"])
    worst = {"L": rel(orc.triple_product(b["A"], b["B"], b["C"]),
                      orc.triple_product(a["A"], a["B"], a["C"]))}
    for key in ("O", "E", "errHist"):
        worst[key] = rel(b[key], a[key])
    print(bc.case_id(case), "nnz(E)=%.3f" % nnz, {k: "%.1e" % v for k, v in worst.items()})
    assert nnz >= 0.20
    assert max(worst.values()) <= 1e-10, worst


@pytest.mark.parametrize("r", bc.SUB_RANKS)
def test_sub_range_problem_is_active_and_well_conditioned(r):
    mod, lib = sc.cref_lib()
    c = sc.e_active_case(r)
    i0, i1 = bc.sub_range(c["D"].shape[0])
    a = bc.sub_reference(r)
    b = sc.as_ref(mod.admm(lib, np.asfortranarray(c["D"][i0:i1]), r, c["opts"],
                           np.asfortranarray(c["A0"][i0:i1]), c["B0"], c["C0"]))
    assert a["k"] == b["k"] == bc.ITERS and a["A"].shape[0] == i1 - i0
    # fewer rows against the same rank: the model fits more and E is sparser
    # than on the whole tensor (r = 4: 5.6 %, ~1150 nonzeros), still active
    assert 0.05 <= sc.nnz_share(a["E"]) <= sc.NNZ_BAND[1]
    worst = {"L": rel(orc.triple_product(b["A"], b["B"], b["C"]),
                      orc.triple_product(a["A"], a["B"], a["C"]))}
    for key in ("O", "E", "A", "B", "C", "errHist"):
        worst[key] = rel(b[key], a[key])
    print("r=%d rows %d..%d" % (r, i0, i1), {k: "%.1e" % v for k, v in worst.items()})
    assert max(worst.values()) <= 1e-11, worst
    # and it is another problem than the whole one: a session that solved the
    # whole tensor, or took A0's first rows, would not pass for it
    whole = sc.oracle_ref(r)
    assert rel(a["B"], whole["B"]) > 1e-3


@pytest.mark.parametrize("case", [("cp", 4), ("f32", 16), ("deg", 2)], ids=["cp4", "f32_16", "deg33x17x1"])
def test_rre_tolerances_catch_a_misread_tensor(case):
    """What the faults the GPU module looks for do to (num, den): one padded
    row summed (as zeros, the mildest form), the last t skipped, X read with
    the contiguous stride from a strided buffer."""
    L = bc.reference_product(case, False)
    n1, n2, n3 = L.shape
    for X in bc.rre_tensors(case, False):
        num, den, rn, rd = bc.rre_reference(L, X)
        Xw = X.astype(np.float64)
        # a row i = n1 of the padded factor (zero) against a finite stand-in for the buffer's next row
        row = Xw[-1]
        bad_row = (num + float(np.sum(row * row)), den + float(np.sum(row * row)))
        if n3 > 1:
            bad_t = bc.rre_reference(L[:, :, :-1], Xw[:, :, :-1])[:2]
        else:
            bad_t = bc.rre_reference(L[:, :-1], Xw[:, :-1])[:2]
        buf, ld, off = bc.padded(Xw, "strided", fill=0.0)
        wrong = buf.ravel(order="K")[:n1 * n2 * n3].reshape((n1, n2, n3), order="F")
        bad_ld = bc.rre_reference(L, wrong)[:2]
        for bn, bd in (bad_row, bad_t, bad_ld):
            assert abs(bn - num) > 1e3 * rn * num or abs(bd - den) > 1e3 * rd * den
