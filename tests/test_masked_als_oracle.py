"""CPU tests of the mask-aware ALS: the masked oracle against its goldens and
against the unmasked oracle, the admission rule of the goldens, and what the
new entry points promise without a device."""
import inspect

import numpy as np
import pytest

import masked_als_cases as mac
import masked_als_oracle as mao
import tritd_oracle as orc
from conftest import load_golden, rel


def quiet(s):
    pass


@pytest.fixture(scope="module")
def reruns():
    """The oracle rerun on every golden's inputs, once."""
    out = {}
    for name in mac.names():
        g = mac.load(name)
        out[name] = (g, mao.triple_decomp_ALS_masked(g["X"], g["observed"], g["r"], g["opts"], g["A0"],
                                                     g["B0"], g["C0"], printer=quiet))
    return out


def test_goldens_present():
    """Every padded rank, the stop case and the three special tiles."""
    names = mac.names()
    assert len(names) >= 8
    assert {mac.padded_rank(mac.load(n)["r"]) for n in names} == {16, 32, 48, 64}


@pytest.mark.parametrize("name", mac.names())
def test_masked_als_oracle_reproduces_golden(reruns, name):
    """Another BLAS or thread count reorders sums: a perturbation below the
    1e-15 the stored drift was measured with, so 10x the drift bounds it."""
    g, (A, B, C, eh, k) = reruns[name]
    assert k == g["k"] and len(eh) == k

    def bound(key):
        return 10.0 * max(float(g[key]), 1e-13)

    for key, X in (("A", A), ("B", B), ("C", C)):
        assert rel(X, g[key]) <= bound("drift_ABC"), key
    assert rel(orc.triple_product(A, B, C), orc.triple_product(g["A"], g["B"], g["C"])) <= bound("drift_L")
    np.testing.assert_allclose(eh, g["errHist"], rtol=bound("drift_errHist"), atol=1e-15)


@pytest.mark.parametrize("name", mac.names())
def test_golden_admission_rule(name):
    """Every tolerance a golden is held to is at least 100x its stored drift,
    and the perturbed reruns stopped at the same k."""
    g = mac.load(name)
    assert float(g["drift_k"]) == 0.0
    for q in mac.held(name):
        key, tol = mac.QUANTITIES[q]
        assert mac.MARGIN * float(g[key]) <= tol, (q, float(g[key]), tol)
    assert "L" in mac.held(name) and "errHist" in mac.held(name)
    assert (~g["observed"]).any() and g["observed"].any()


def test_every_padded_rank_has_a_golden_held_for_the_factors():
    held = {mac.padded_rank(mac.load(n)["r"]) for n in mac.names() if "ABC" in mac.held(n)}
    assert held == {16, 32, 48, 64}


@pytest.mark.parametrize("name", mac.names())
def test_errhist_never_increases(name):
    """Each iteration is an EM step of the masked least-squares fit (up to the
    1e-9 ridge)."""
    eh = mac.load(name)["errHist"]
    assert (eh[1:] <= eh[:-1] * (1.0 + 1e-12)).all()


def test_stop_golden_stops_early_with_the_factors_un_updated(reruns):
    g, (A, B, C, eh, k) = reruns["oals12x10x8_r2_stop"]
    assert 1 < g["k"] < g["opts"]["maxIter"]
    # errHist(k) is the error of the returned factors: they were not updated after it
    Xo = np.where(g["observed"], g["X"], 0.0)
    L = orc.triple_product(A, B, C)
    e = np.linalg.norm(np.where(g["observed"], Xo - L, 0.0).ravel()) / np.linalg.norm(Xo.ravel())
    assert abs(e - eh[-1]) <= 1e-12 * eh[-1]


def test_tiles_golden_has_the_three_special_tiles():
    obs = mac.load("oals30_r3_tiles")["observed"]
    assert obs[:16, 0, :16].sum() == 0
    assert obs[:16, 1, :16].sum() == 1
    assert obs[:16, 2, :16].sum() == 255


@pytest.mark.parametrize("name", ["als12x10x8_r2", "als17x16x20_r8", "als20x24x18_r5_stop"])
def test_all_true_mask_is_the_reference_bitwise(name):
    g = load_golden(name)
    ref = orc.triple_decomp_ALS(g["X"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"], printer=quiet)
    for observed in (None, np.ones(g["X"].shape, dtype=bool)):
        got = mao.triple_decomp_ALS_masked(g["X"], observed, g["r"], g["opts"], g["A0"], g["B0"],
                                           g["C0"], printer=quiet)
        assert got[4] == ref[4]
        for a, b in zip(got[:4], ref[:4]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["oals12x10x8_r2_stop", "oals21x13x35_r5"])
def test_fill_values_never_enter(reruns, name):
    g, ref = reruns[name]
    for fill in (np.nan, np.inf, 1e30):
        X = g["X"].copy(order="F")
        X[~g["observed"]] = fill
        got = mao.triple_decomp_ALS_masked(X, g["observed"], g["r"], g["opts"], g["A0"], g["B0"],
                                           g["C0"], printer=quiet)
        assert got[4] == ref[4]
        for a, b in zip(got[:4], ref[:4]):
            np.testing.assert_array_equal(a, b)


def test_progress_line_every_five_iterations():
    g = mac.load("oals12x10x8_r2")
    lines = []
    _, _, _, eh, k = mao.triple_decomp_ALS_masked(g["X"], g["observed"], g["r"], g["opts"], g["A0"],
                                                  g["B0"], g["C0"], printer=lines.append)
    assert lines == ["Iteration %d, relative error = %.4e" % (i, eh[i - 1]) for i in range(5, k + 1, 5)]


# ---------------------------------------------------------------------------
# the new entry points, without a device
# ---------------------------------------------------------------------------
def test_new_symbols_are_bound_with_the_documented_signatures():
    import ctypes as C

    import tritd
    from tritd import _lib
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    for name in ("tritd_als_masked_f64", "tritd_als_session_create_masked",
                 "tritd_als_session_mask_info"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert _lib.SIGNATURES[name][0] is C.c_int
    # the masked forms take the unmasked forms' arguments plus `observed` after X
    one = list(_lib.SIGNATURES["tritd_als_f64"][1])
    assert _lib.SIGNATURES["tritd_als_masked_f64"][1] == one[:1] + [vp] + one[1:]
    ses = list(_lib.SIGNATURES["tritd_als_session_create"][1])
    assert _lib.SIGNATURES["tritd_als_session_create_masked"][1] == ses[:3] + [vp] + ses[3:]
    assert _lib.SIGNATURES["tritd_als_session_mask_info"][1] == [vp, C.POINTER(i32), C.POINTER(i64)]
    assert inspect.signature(tritd.triple_decomp_ALS).parameters["observed"].default is None
    assert inspect.signature(tritd.AlsSession.__init__).parameters["observed"].default is None
    assert callable(tritd.AlsSession.mask_info)


def test_header_declares_the_new_entry_points():
    import os

    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "tritd.h")).read()
    for name in ("tritd_als_masked_f64", "tritd_als_session_create_masked",
                 "tritd_als_session_mask_info"):
        assert ("tritd_status %s(" % name) in h


def test_observed_shape_mismatch_raises():
    import tritd
    g = mac.load("oals12x10x8_r2")
    with pytest.raises(ValueError, match="observed must have the shape of X"):
        tritd.triple_decomp_ALS(g["X"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                observed=g["observed"][:, :, :-1])
    with pytest.raises(ValueError, match="observed must have the shape of X"):
        tritd.AlsSession(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=12, n2=10, n3=8, X=g["X"],
                         observed=g["observed"].ravel())


def test_observed_with_virtual_shards_raises():
    import tritd
    g = mac.load("oals12x10x8_r2")
    with pytest.raises(ValueError, match=r"set_devices\(\[d\] \* P\)"):
        tritd.triple_decomp_ALS(g["X"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                observed=g["observed"], virtual_shards=2)
