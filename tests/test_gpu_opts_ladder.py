"""The robust ADMM and the nonconvex solver on the GPU across their option space.

Every other GPU parity test runs at mu = 1e-3, rho = 1.25, lambda2 = 1e-3 (or
rho = 1.05, or the video configuration's mu = 1e-2, rho = 1.2), where K5's
host-derived scalars never leave one pattern: cprev = mu_[k-2]/mu_[k-1] is
always 0.8 and the clip of the mu schedule never acts.  Here the ladder of
tests/opts_cases.py (13 regimes: constant, falling, saturating and clipped
schedules, mu from 1e-7 to 10, lambda2 from 0 to 10, lambda 0 and 1e30) runs on
the sweep's inputs (ragged ~35 x 20 x 33), against the numpy oracle at the
tolerances of tests/test_gpu_parity.py through test_gpu_rank_sweep.check,
unchanged (L, O, E <= 1e-9; A, B, C <= 1e-8; errHist rtol 1e-8 atol 1e-11; same
k).  tests/test_opts_cases.py admits every cell on the CPU (the references move
by at most 1.6e-12 under a 1e-14 perturbation of D).

Forms: one-shot at r = 5, 8, 11 (padded rank 32, 64, 128); a Session stepped
3 + rest at r = 5, read after both steps (the O fix-up of get() then runs
mid-schedule with that regime's invL_next); the 70 % mask at r = 5 against
tests/masked_oracle.py; five regimes under TRITD_FUSED=0, TRITD_DENSE_E=1, a
device set of one GPU three times (r = 6) and the Qi model; fp32 at r = 4 and
r = 16 against the class-single C restatement with test_gpu_f32's TOL, EH_C and
RHO (opts_cases.F32_CELLS: all 13 regimes at r = 4, three of the nine admitted
ones at r = 16); the ten rows of the nonconvex table
plain and masked at the tolerances of tests/test_ncvx.py; and the session's
own switch to dense-E storage, unforced, after iteration 24, after iteration 8
and not at all.

Measured on an MI355X (profiles/opts_ladder/gpu_opts_ladder.txt): the worst
relative deviation of L, O, E per form, and the worst relative errHist
deviation of the regime over all its forms (sat_clip's 3e-12 is at an errHist
of 1e-10, inside atol).  "3" is the session read after 3 iterations, "3+" the
same session at the end, "side" TRITD_FUSED=0, "dense" TRITD_DENSE_E=1, "devs"
set_devices([0,0,0]) at r = 6:
  regime     r=5    r=8    r=11   3      3+     masked side   dense  devs   qi     errHist
  rho1       4e-14  1e-13  2e-13  8e-15  4e-14  3e-14  4e-14  4e-14  4e-13  5e-14  3e-14
  rho1_lam1  4e-13  1e-13  1e-13  8e-15  4e-13  2e-14  4e-13  4e-13  3e-14  2e-14  7e-14
  rho_dec    4e-13  3e-13  9e-13  7e-15  4e-13  9e-14  4e-13  4e-13  3e-13  7e-14  2e-14
  sat_fast   9e-15  6e-15  8e-15  6e-15  9e-15  7e-15  -      -      -      -      4e-16
  sat_mid    1e-14  8e-15  9e-15  7e-15  1e-14  9e-15  -      -      -      -      2e-14
  sat_clip   2e-14  9e-15  1e-14  6e-15  2e-14  1e-14  2e-14  2e-14  1e-14  1e-14  3e-12
  mu_small   1e-14  3e-14  3e-14  8e-15  1e-14  4e-14  -      -      -      -      2e-15
  mu_large   2e-14  2e-14  3e-14  8e-15  2e-14  4e-14  -      -      -      -      5e-15
  mu1_rho1   4e-14  1e-13  2e-13  8e-15  4e-14  3e-14  -      -      -      -      2e-14
  lam2_zero  2e-14  2e-14  3e-14  8e-15  2e-14  8e-15  -      -      -      -      5e-15
  lam2_big   1e-14  2e-14  3e-14  8e-15  1e-14  1e-14  -      -      -      -      3e-15
  lam_zero   1e-14  8e-15  8e-15  8e-15  1e-14  2e-14  1e-14  1e-14  9e-15  1e-14  6e-14
  lam_huge   6e-14  9e-14  1e-13  7e-15  6e-14  2e-14  -      -      -      -      1e-15
A, B, C: at most 5.7e-13 (rho1_lam1, side-stream schedule).  fp32, worst of
rel L, O, E (TOL 2e-5) / largest |d errHist| as a fraction of its bound, no
cell needing any rho (rho_needed = 0 everywhere, so RHO stays as it is):
  regime     r=4              r=16
  rho1       4.7e-7 / 0.012   (not admitted)
  rho1_lam1  8.3e-7 / 0.070   (not admitted)
  rho_dec    2.3e-6 / 0.012   (not admitted)
  sat_fast   2.1e-7 / 0.000   8.5e-7 / 0.003
  sat_mid    2.3e-7 / 0.001   1.1e-6 / 0.001
  sat_clip   2.4e-7 / 0.001   1.4e-6 / 0.002
  mu_small   1.5e-7 / 0.007   5.1e-6 / 0.003
  mu_large   1.5e-7 / 0.006   5.1e-6 / 0.006
  mu1_rho1   1.5e-6 / 0.010   (not admitted)
  lam2_zero  1.5e-7 / 0.000   4.9e-6 / 0.010
  lam2_big   1.4e-7 / 0.007   4.9e-6 / 0.003
  lam_zero   2.7e-7 / 0.002   8.3e-7 / 0.001
  lam_huge   4.8e-7 / 0.006   6.3e-6 / 0.007
Nonconvex rows, plain and masked: A, B, C, O, L at most 2.7e-14, errHist within
6.7e-16 absolute.  Dense-E switch: storage forms (4, 3) after 10 and (7, 0)
after 26 iterations; parity after the switch at 24 L, O, E 7.8e-15, A, B, C
3.1e-14; the forced, refused and self-switched forms are equal bit for bit.
An r = 16 fp32 cell takes ~14 s, nearly all of it the C restatement's reference
on the host (1.4 s per iteration at R = 256): the nine above were measured in
one run of all of them (profiles/opts_ladder/gpu_opts_ladder_all_r16.txt) and
the suite keeps sat_clip, mu_small and lam_huge (opts_cases.F32_R16_IN_SUITE).
"""
import numpy as np
import pytest

import masked_ncvx_cases as mnc
import opts_cases as oc
import sweep_cases as sc
from conftest import rel
from test_gpu_f32 import _compare
from test_gpu_rank_sweep import check, session_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    t.set_printer(lambda s: None)
    yield t
    t.set_printer(None)


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


@pytest.fixture(autouse=True)
def storage_form_unforced(monkeypatch):
    monkeypatch.delenv("TRITD_DENSE_E", raising=False)


def solve(tritd, c, **kw):
    return tritd.triple_decomp_ADMM(c["D"], c["r"], c["opts"], c["A0"], c["B0"], c["C0"],
                                    return_E=True, return_iters=True, **kw)


def session(tritd, c):
    n1, n2, n3 = c["D"].shape
    return tritd.Session(c["r"], c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                         D=c["D"], device=0)


def ladder_check(orc, got, regime, r, label, ref=None, model="cp"):
    check(orc, got, "%d %s" % (r, regime), label, ref=oc.ref(regime, r, model) if ref is None else ref,
          e_zero=regime == "lam_huge", model=model)


# --- 1. the ladder, fp64 CP ----------------------------------------------------
@pytest.mark.parametrize("r", oc.RANKS)
@pytest.mark.parametrize("regime", oc.IDS)
def test_one_shot(tritd, orc, regime, r):
    ladder_check(orc, solve(tritd, oc.case(regime, r)), regime, r, "one-shot")


@pytest.mark.parametrize("regime", oc.IDS)
def test_session_read_mid_schedule(tritd, orc, regime):
    """3 + rest iterations, get() after both steps: O is rebuilt from
    (D + invL_next Y_L) - T with the invL_next of iteration 3, inside the
    transient of the saturating regimes."""
    r = oc.R_FORMS
    s = session(tritd, oc.case(regime, r))
    try:
        s.run(3)
        early = session_result(s)
        s.run(oc.iters(regime) - 3)
        late = session_result(s)
    finally:
        s.close()
    # (after 3 iterations E is still all zero in some regimes only because lambda says so)
    check(orc, early, "%d %s" % (r, regime), "session after 3", ref=oc.ref(regime, r, "cp", 3),
          e_zero=regime == "lam_huge")
    ladder_check(orc, late, regime, r, "session 3+%d" % (oc.iters(regime) - 3))


@pytest.mark.parametrize("regime", oc.IDS)
def test_masked(tritd, orc, regime):
    r = oc.R_FORMS
    obs = oc.observed(r)
    got = solve(tritd, oc.case(regime, r), observed=obs)
    ladder_check(orc, got, regime, r, "masked", ref=oc.masked_ref(regime, r))
    O, E = got[3], got[5]
    assert not O[~obs].any() and not E[~obs].any()


@pytest.mark.parametrize("regime", oc.SUBSET)
def test_side_stream_schedule(tritd, orc, regime, monkeypatch):
    monkeypatch.setenv("TRITD_FUSED", "0")
    ladder_check(orc, solve(tritd, oc.case(regime, oc.R_FORMS)), regime, oc.R_FORMS, "TRITD_FUSED=0")


@pytest.mark.parametrize("regime", oc.SUBSET)
def test_dense_e_form(tritd, orc, regime, monkeypatch):
    monkeypatch.setenv("TRITD_DENSE_E", "1")
    c = oc.case(regime, oc.R_FORMS)
    ladder_check(orc, solve(tritd, c), regime, oc.R_FORMS, "TRITD_DENSE_E=1")
    s = session(tritd, c)
    try:
        s.run(1)
        s.sync()
        assert s.k5_profile() == (7, 0)  # dense E streams, no slot accesses: the form really ran
    finally:
        s.close()


@pytest.mark.parametrize("regime", oc.SUBSET)
def test_device_set(tritd, orc, regime):
    r = oc.R_DEVICE_SET
    tritd.set_devices([0, 0, 0])
    try:
        got = solve(tritd, oc.case(regime, r))
    finally:
        tritd.set_devices([])
    ladder_check(orc, got, regime, r, "set_devices([0,0,0])")


@pytest.mark.parametrize("regime", oc.SUBSET)
def test_qi_model(tritd, orc, regime):
    r = oc.R_FORMS
    c = oc.case(regime, r, model="qi")
    assert c["opts"]["model"] == "qi"
    ladder_check(orc, solve(tritd, c), regime, r, "qi", model="qi")


# --- 2. fp32 -------------------------------------------------------------------
@pytest.mark.parametrize("regime, r", oc.F32_CELLS)
def test_f32(tritd, capsys, regime, r):
    """The cells tests/test_opts_cases.py admits, through test_gpu_f32._compare
    with that module's TOL, EH_C and RHO."""
    c = oc.case(regime, r, np.float32)
    ref = oc.c_ref32(regime, r)
    ref = (ref["A"], ref["B"], ref["C"], ref["O"], ref["errHist"], ref["E"], ref["k"])
    assert bool(np.any(ref[5])) == (regime != "lam_huge")
    rep = {}
    try:
        _compare(tritd, sc.cref_lib(), c["D"], r, c["opts"], c["A0"], c["B0"], c["C0"], ref=ref, report=rep)
    finally:
        with capsys.disabled():
            print("  f32 ladder r=%d %s: %s" % (r, regime, {k: (float("%.3g" % v) if isinstance(v, float) else v)
                                                            for k, v in rep.items()}), flush=True)


# --- 3. the nonconvex solver ---------------------------------------------------
def ncvx_check(orc, got, ref, what, obs=None):
    """The comparisons of test_ncvx._check / test_gpu_masked_ncvx.check (A, B, C,
    O, triple_product <= 1e-9, errHist rtol 1e-8 atol 1e-13, same k), every
    figure printed before it is asserted."""
    A, B, C, O, eh, k = got
    fig = dict(k=k, L=rel(orc.triple_product(A, B, C), orc.triple_product(ref["A"], ref["B"], ref["C"])))
    for key, X in (("A", A), ("B", B), ("C", C), ("O", O)):
        fig[key] = rel(X, ref[key])
    n = min(len(eh), len(ref["errHist"]))
    fig["errHist(abs)"] = float(np.max(np.abs(eh[:n] - ref["errHist"][:n])))
    print("  ncvx", what, "nnz(O)=%.3f nnz(A)=%.3f" % (sc.nnz_share(O), sc.nnz_share(A)),
          " ".join("%s=%.2e" % kv for kv in fig.items()), flush=True)
    for key in ("L", "A", "B", "C", "O"):
        assert fig[key] <= mnc.TOL, key
    assert k == ref["k"] and len(eh) == len(ref["errHist"])
    np.testing.assert_allclose(eh, ref["errHist"], rtol=mnc.RTOL_ERR, atol=mnc.ATOL_ERR)
    if obs is not None:
        assert not O[~obs].any()


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("row", oc.NCVX_IDS)
def test_ncvx(tritd, orc, row, masked):
    c = sc.e_active_case(oc.NCVX_R)
    obs = oc.observed(oc.NCVX_R) if masked else None
    ref = oc.ncvx_ref(row, masked)
    assert bool(np.any(ref["O"])) == (row != "lam_huge")
    got = tritd.triple_decomp_ncvx(c["D"], oc.NCVX_R, *oc.ncvx_args(row), c["A0"], c["B0"], c["C0"],
                                   return_iters=True, observed=obs)
    assert bool(np.any(got[3])) == (row != "lam_huge")
    ncvx_check(orc, got, ref, "%s %s" % (row, "masked" if masked else "plain"), obs)


# --- 4. the session's own switch to dense-E storage ----------------------------
COMPACT, DENSE = (4, 3), (7, 0)  # Session::k5_profile of an fp64 session in either form


def run_switch_case(tritd, cfg):
    """Runs cfg's steps; returns (result, the storage form after each step,
    the form the launch after the run used)."""
    s = session(tritd, oc.switch_case(cfg["regime"], cfg["n"]))
    try:
        forms = []
        for n in cfg["steps"]:
            s.run(n)
            s.sync()
            forms.append(s.k5_profile())
        got = session_result(s)
        s.run(1)
        s.sync()
        return got, forms, s.k5_profile()
    finally:
        s.close()


def switch_check(orc, got, cfg, label):
    check(orc, got, "%d %s" % (oc.SWITCH_R, cfg["regime"]), label, ref=oc.switch_ref(cfg["regime"], cfg["n"]))


def test_switch_at_24(tritd, orc):
    """The dense-tile share is 0.24 over iterations 1-8 and 0.60 over 9-24: the
    check after iteration 8 passes over, the one after 24 expands E^(24) and
    E^(23) and K5 runs its dense-E form from 25 on."""
    got, forms, after = run_switch_case(tritd, oc.SWITCH24)
    print("  storage forms after the steps %s: %s, then %s" % (oc.SWITCH24["steps"], forms, after))
    switch_check(orc, got, oc.SWITCH24, "10+16, switch at 24")
    assert forms == [COMPACT, DENSE] and after == DENSE


def test_switch_at_8(tritd, orc):
    got, forms, after = run_switch_case(tritd, oc.SWITCH8)
    switch_check(orc, got, oc.SWITCH8, "12, switch at 8")
    assert forms == [DENSE] and after == DENSE


def test_no_switch(tritd, orc):
    got, forms, after = run_switch_case(tritd, oc.NO_SWITCH)
    switch_check(orc, got, oc.NO_SWITCH, "26, no switch")
    assert forms == [COMPACT] and after == COMPACT


def test_switch_is_storage_only(tritd, monkeypatch):
    """The switch-at-24 run (26 iterations in one step) against the same session
    with the dense form forced from the start and with it refused: A, B, C, O,
    errHist and E are equal bit for bit (measured so on an MI355X; the parity
    tests only ever held the two forms to check's tolerances)."""
    cfg = dict(oc.SWITCH24, steps=(oc.SWITCH24["n"],))
    own, forms, _ = run_switch_case(tritd, cfg)
    assert forms == [DENSE]
    for forced, form in (("1", DENSE), ("0", COMPACT)):
        monkeypatch.setenv("TRITD_DENSE_E", forced)
        got, forms, _ = run_switch_case(tritd, cfg)
        assert forms == [form]
        fig = {key: rel(x, y) for key, x, y in zip(("A", "B", "C", "O", "errHist", "E"), got, own)}
        print("  TRITD_DENSE_E=%s against the session's own switch: " % forced
              + " ".join("%s=%.1e" % kv for kv in fig.items()), flush=True)
        assert got[6] == own[6]
        for x, y in zip(got[:6], own[:6]):
            np.testing.assert_array_equal(x, y)
