"""CPU: the truncated-pinv cases (tests/pinv_cases.py) are what
tests/test_gpu_pinv_fallback.py takes them for.  From the references alone,
for every case:

  * clean truncation: every Gram of the reference run either drops nothing or
    drops values all <= 0.5 x pinv's cutoff while keeping values all >= 1e6 x
    the cutoff; every Gram has max sigma / min kept <= 1e7 (the bar
    tests/test_gpu_flags.py states for its 1e-8); the named update drops the
    tabulated number of values in the tabulated iterations;
  * two independent CPU references agree to <= 1e-10 (a hundredth of the GPU
    tolerance) in every quantity the GPU test compares: the numpy oracle (SVD
    pinv) against the C restatement (Jacobi pinv_sym) for fp64 ADMM, against
    itself with an eigh-based pinv for ALS, the nonconvex solver and Qi;
  * the case discriminates: with numpy.linalg.inv in pinv's place (what a GPU
    that skipped the fallback computes) the oracle lands >= 1e-5 away (1000 x
    the GPU tolerance; >= 2e-2 for the float32 cases, 1000 x theirs) in at
    least one compared quantity, non-finite output and a singular Gram
    counting as different;
  * float32: the class-single restatement moves by <= 5e-6 in L and O (a
    quarter of test_gpu_f32.TOL) when X is perturbed by one unit of single;
  * exact fits: the reference's last errHist is < 1e-10 exactly where the
    table says so (every C_trunc and ABC_trunc case, no A_* case); the GPU
    test compares O, E and errHist absolutely there.
"""
import numpy as np
import pytest

import pinv_cases as pc
import sweep_cases as sc
from conftest import rel

import tritd_oracle as orc

U32 = 2.0 ** -24

# (update, iteration) -> values dropped, per case, as the spy counts them
DROPS = {
    "A_small_r4": {("A", 1): 7}, "A_small_r5": {("A", 1): 9}, "A_small_r6": {("A", 1): 20},
    "A_small_r7": {("A", 1): 29}, "A_small_r8": {("A", 1): 39},
    "A_rows_r4": {("A", 1): 7}, "A_rows_r8": {("A", 1): 39}, "A_rows_r6": {("A", 1): 20},
    "A_wide_r9": {("A", 1): 56}, "A_wide_r11": {("A", 1): 96}, "A_wide_r12": {("A", 1): 108},
    "A_wide_r16": {("A", 1): 192},
    "C_trunc_r5": {("C", 1): 9, ("C", 2): 9}, "C_trunc_r8": {("C", 1): 39, ("C", 2): 39},
    "C_trunc_r8_rows": {("C", 1): 39, ("C", 2): 39}, "C_trunc_r4_rows": {("C", 1): 7, ("C", 2): 7},
    "C_trunc_r9": {("C", 1): 56, ("A", 2): 6, ("C", 2): 56},
    "C_trunc_r16": {("C", 1): 192, ("C", 2): 192},
    "ABC_trunc_admm": {("C", 1): 5, ("A", 2): 3, ("B", 2): 1, ("C", 2): 5},
    "ABC_trunc_als": {("C", 1): 5, ("A", 2): 3, ("B", 2): 1, ("C", 2): 5},
    "ALS_A_r6": {("A", 1): 20, ("A", 2): 20}, "ALS_A_r8": {("A", 1): 39, ("A", 2): 39},
    "ALS_C_r4": {("C", 1): 7, ("C", 2): 7}, "ALS_C_r5": {("C", 1): 9, ("C", 2): 9},
    "ALS_C_r8": {("C", 1): 39, ("C", 2): 39},
    "F32_r4": {("A", 1): 7}, "F32_r8": {("A", 1): 39}, "F32_r9": {("A", 1): 56},
    "F32_r16": {("A", 1): 192},
    "opt_qi_r6": {("A", 1): 20}, "opt_ncvx_r6": {("A", 1): 20, ("A", 2): 20},
    "devset_r4": {("A", 1): 7}, "devset_r5": {("A", 1): 9}, "devset_r6": {("A", 1): 20},
    "devset_r7": {("A", 1): 29}, "devset_r8": {("A", 1): 39},
    "devset_C_r5": {("C", 1): 9, ("C", 2): 9}, "devset_C_r8": {("C", 1): 39, ("C", 2): 39},
    "devset_ABC_r3": {("C", 1): 5, ("A", 2): 3, ("B", 2): 1, ("C", 2): 5},
}

ALL = list(pc.CASES)
F64 = [n for n in ALL if pc.CASES[n].dtype == np.float64]


def test_table_covers_every_padded_rank_and_consumer():
    assert set(DROPS) == set(pc.CASES)
    rp = lambda g: sorted(pc.padded_rank(pc.CASES[n].r) for n in pc.GROUPS[g])  # noqa: E731
    assert rp("A_small") == [16, 32, 48, 64, 64]
    assert rp("A_wide") == [128, 128, 256, 256] and rp("F32") == [16, 64, 128, 256]
    for n in pc.GROUPS["A_small"]:
        c = pc.CASES[n]
        assert -(-c.shape[0] // 16) * 16 * pc.padded_rank(c.r) ** 2 <= 327680
    for n in pc.GROUPS["A_rows"]:
        c = pc.CASES[n]
        assert c.shape[0] * pc.padded_rank(c.r) ** 2 > 327680
    assert {pc.padded_rank(pc.CASES[n].r) for n in pc.GROUPS["A_rows"]} == {16, 48, 64}
    for c in pc.CASES.values():
        assert np.prod(c.shape) < 20000


@pytest.mark.parametrize("name", ALL)
def test_every_gram_is_cleanly_truncated_or_untouched(name):
    case = pc.CASES[name]
    ref, calls = pc.spied(name)
    assert len(calls) == 3 * ref["k"] == 3 * case.iters
    drops = {}
    for i, c in enumerate(calls):
        u, it = pc.call_label(i)
        print("%s %s(%d): dropped %d, max dropped %.3g x cutoff, min kept %.3g x cutoff, "
              "sigma max / min kept %.3g" % (name, u, it, c["dropped"], c["max_dropped"],
                                             c["min_kept"], c["cond_kept"]))
        if c["dropped"]:
            drops[(u, it)] = c["dropped"]
            assert c["max_dropped"] <= pc.DROP_MAX and c["min_kept"] >= pc.KEEP_MIN, (u, it, c)
        assert c["cond_kept"] <= pc.COND_MAX, (u, it, c)
    assert drops == DROPS[name]
    assert {u for u, _ in drops} >= set(case.trunc)


@pytest.mark.parametrize("name", F64)
def test_two_cpu_references_agree(name):
    ref, other = pc.reference(name), pc.second_reference(name)
    assert ref["k"] == other["k"] == pc.CASES[name].iters
    f = pc.figures(name, other, ref)
    print(name, "reference spread", {k: "%.1e" % v for k, v in f.items()})
    assert max(f.values()) <= pc.REF_SPREAD, f


@pytest.mark.parametrize("name", ALL)
def test_an_inverse_in_place_of_pinv_lands_elsewhere(name):
    case = pc.CASES[name]
    ref = pc.spied(name)[0]
    try:
        with np.errstate(all="ignore"):
            f = pc.figures(name, pc.run_oracle(name, pc.plain_inverse), ref)
    except np.linalg.LinAlgError:
        f = {"singular": float("inf")}
    print(name, "inverse instead of pinv", {k: "%.1e" % v for k, v in f.items()})
    assert max(f.values()) >= pc.INV_GAP * (2e3 if case.dtype == np.float32 else 1.0), f


@pytest.mark.parametrize("name", pc.GROUPS["F32"])
def test_fp32_restatement_is_stable_under_input_rounding(name):
    base = pc.reference(name)
    X = pc.inputs(name)[0]
    assert X.dtype == np.float32 and base["O"].dtype == np.float32
    L0 = orc.triple_product(base["A"], base["B"], base["C"])
    worst = 0.0
    for seed in (1, 2, 3):
        p = pc.run_cref(name, sc.perturbed(X, U32, np.random.default_rng(seed)))
        assert p["k"] == base["k"]
        worst = max(worst, rel(orc.triple_product(p["A"], p["B"], p["C"]), L0),
                    rel(p["O"].astype(np.float64), base["O"].astype(np.float64)))
    print("%s fp32 perturbation response %.2e" % (name, worst))
    assert worst <= 5e-6


@pytest.mark.parametrize("name", ALL)
def test_exact_fit_flag(name):
    case = pc.CASES[name]
    last = float(pc.spied(name)[0]["errHist"][-1])
    print("%s last errHist %.3g: %s" % (name, last, "exact fit" if case.exact else "not exact"))
    assert pc.is_exact_fit(pc.spied(name)[0]) == case.exact
    assert case.exact == (case.trunc in ("C", "ABC"))
    if case.group.startswith("A_"):
        assert not case.exact
