"""CPU tests of the held-out validation error of the masked ALS: the holdout
oracle against the masked oracle and against its goldens, the admission and
decision-margin rules of the goldens, the rank-selection case, and what the
new entry points promise without a device."""
import inspect

import numpy as np
import pytest

import holdout_als_cases as hac
import holdout_als_oracle as hao
import masked_als_oracle as mao
import tritd_oracle as orc
from conftest import rel


def quiet(s):
    pass


def run(g, **kw):
    a = dict(X=g["X"], observed=g["observed"], holdout=g["holdout"], opts=g["opts"], patience=g["patience"])
    a.update(kw)
    return hao.triple_decomp_ALS_holdout(a["X"], a["observed"], a["holdout"], g["r"], a["opts"], g["A0"],
                                         g["B0"], g["C0"], a["patience"], quiet)


@pytest.fixture(scope="module")
def reruns():
    """The oracle rerun on every golden's inputs, once."""
    return {name: (g, run(g)) for name, g in ((n, hac.load(n)) for n in hac.names())}


def test_goldens_present():
    """Every padded rank, the five t-tiles, the tiles and the ragged shape."""
    bases = {str(hac.load(n)["base"]) for n in hac.names()}
    assert {"oals20x6x70_r3", "oals30_r3_tiles", "oals19x21x23_r7"} <= bases
    assert {hac.padded_rank(hac.load(n)["r"]) for n in hac.names()} == {16, 32, 48, 64}


def test_goldens_cover_every_way_to_stop():
    g = {n: hac.load(n) for n in hac.names()}
    assert any(x["stop_reason"] == 2 and x["patience"] > 0 and 1 < x["best_iter"] < x["k"] and
               x["k"] - x["best_iter"] == x["patience"] for x in g.values())
    assert any(x["stop_reason"] == 1 and x["k"] < x["opts"]["maxIter"] for x in g.values())
    assert any(x["stop_reason"] == 0 and x["k"] == x["opts"]["maxIter"] for x in g.values())
    # a patience that is set and never fires
    assert any(x["stop_reason"] == 0 and x["patience"] > 0 for x in g.values())


@pytest.mark.parametrize("name", hac.names())
def test_patience_zero_is_the_masked_oracle_bitwise(name):
    g = hac.load(name)
    got = run(g, patience=0)
    ref = mao.triple_decomp_ALS_masked(g["X"], g["fit"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                       printer=quiet)
    assert got[4] == ref[4]
    for a, b in zip(got[:4], ref[:4]):
        np.testing.assert_array_equal(a, b)
    assert got[5]["stop_reason"] == (1 if got[4] < g["opts"]["maxIter"] else 0)


@pytest.mark.parametrize("name", ["hals17x16x20_r8_p3", "hals20x6x70_r3"])
def test_valhist_is_the_error_of_the_factors_the_iteration_started_with(reruns, name):
    g, (_, _, _, _, k, info) = reruns[name]
    H = g["held_out"]
    for kk in (1, 2, info["best_iter"], k):
        A, B, C, _, _ = mao.triple_decomp_ALS_masked(g["X"], g["fit"], g["r"], dict(maxIter=kk - 1, tol=0.0),
                                                     g["A0"], g["B0"], g["C0"], printer=quiet)
        L = orc.triple_product(A, B, C)
        ref = np.linalg.norm((g["X"] - L)[H]) / np.linalg.norm(g["X"][H])
        assert abs(info["valHist"][kk - 1] - ref) <= 1e-13 * ref, kk
        if kk == info["best_iter"]:
            for x, y in ((A, info["A_best"]), (B, info["B_best"]), (C, info["C_best"])):
                np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", hac.names())
def test_holdout_oracle_reproduces_golden(reruns, name):
    """Another BLAS or thread count reorders sums: a perturbation below the
    1e-15 the stored drift was measured with, so 10x the drift bounds it."""
    g, (A, B, C, eh, k, info) = reruns[name]
    assert k == g["k"] and len(eh) == k and len(info["valHist"]) == k
    assert info["best_iter"] == g["best_iter"] and info["stop_reason"] == g["stop_reason"]
    assert info["holdout_count"] == int(g["holdout_count"]) == int(g["held_out"].sum())

    def bound(key):
        return 10.0 * max(float(g[key]), 1e-13)

    for key, X in (("A", A), ("B", B), ("C", C), ("A_best", info["A_best"]), ("B_best", info["B_best"]),
                   ("C_best", info["C_best"])):
        assert rel(X, g[key]) <= bound("drift_ABC"), key
    assert rel(orc.triple_product(A, B, C), orc.triple_product(g["A"], g["B"], g["C"])) <= bound("drift_L")
    np.testing.assert_allclose(eh, g["errHist"], rtol=bound("drift_errHist"), atol=1e-15)
    np.testing.assert_allclose(info["valHist"], g["valHist"], rtol=bound("drift_valHist"), atol=1e-15)


@pytest.mark.parametrize("name", hac.names())
def test_golden_admission_rule(name):
    """Every tolerance a golden is held to is at least 100x its stored drift
    (valHist at TOL_ERR included), and the perturbed reruns took the same k,
    best_iter and stop_reason."""
    g = hac.load(name)
    assert float(g["drift_k"]) == 0.0
    for q in hac.held(name):
        key, tol = hac.QUANTITIES[q]
        assert hac.MARGIN * float(g[key]) <= tol, (q, float(g[key]), tol)
    assert {"L", "errHist", "valHist"} <= set(hac.held(name))
    assert g["held_out"].any() and g["fit"].any() and (~g["observed"]).any()
    assert (g["holdout"] & ~g["observed"]).any()  # flags outside Omega are in every golden


@pytest.mark.parametrize("name", hac.names())
def test_every_deciding_comparison_has_a_margin(name):
    """valHist(k) against the running best differs by >= 1e-6 relative, 1000x
    TOL_ERR: a result inside the tolerance cannot flip best_iter or the stop."""
    g = hac.load(name)
    assert hac.DECISION_MARGIN / hac.TOL_ERR >= 1000.0 * (1.0 - 1e-12)  # (1000 * 1e-9 rounds above 1e-6)
    m = hac.decision_margins(g["valHist"])
    assert len(m) == g["k"] - 1 and (m >= hac.DECISION_MARGIN).all(), m.min()
    assert g["best_iter"] == int(np.argmin(g["valHist"])) + 1


def test_patience_stop_returns_the_factors_un_updated(reruns):
    g, (A, B, C, eh, k, info) = reruns["hals17x16x20_r8_p3"]
    assert info["stop_reason"] == 2 and k < g["opts"]["maxIter"]
    ref = mao.triple_decomp_ALS_masked(g["X"], g["fit"], g["r"], dict(maxIter=k - 1, tol=0.0), g["A0"],
                                       g["B0"], g["C0"], printer=quiet)
    for a, b in zip((A, B, C), ref[:3]):
        np.testing.assert_array_equal(a, b)
    # the same run without patience goes on, with the same history up to k
    _, _, _, eh0, k0, info0 = run(g, patience=0)
    assert k0 == g["opts"]["maxIter"] > k
    np.testing.assert_array_equal(eh0[:k], eh)
    np.testing.assert_array_equal(info0["valHist"][:k], info["valHist"])


def test_flags_outside_observed_and_fill_values_never_enter(reruns):
    g, ref = reruns["hals12x10x8_r2_stop"]
    for fill in (np.nan, np.inf, 1e30):
        X = g["X"].copy(order="F")
        X[~g["observed"]] = fill
        got = run(g, X=X, holdout=g["held_out"] | ~g["observed"])
        assert got[4] == ref[4] and got[5]["best_iter"] == ref[5]["best_iter"]
        for a, b in zip(got[:4] + (got[5]["valHist"],), ref[:4] + (ref[5]["valHist"],)):
            np.testing.assert_array_equal(a, b)


def test_oracle_refusals():
    g = hac.load("hals12x10x8_r2_stop")
    X0 = g["X"].copy(order="F")
    X0[g["held_out"]] = 0.0
    for kw in (dict(holdout=~g["observed"]), dict(holdout=np.ones(g["X"].shape, dtype=bool)), dict(X=X0),
               dict(patience=-1)):
        with pytest.raises(ValueError):
            run(g, **kw)


# ---------------------------------------------------------------------------
# the rank-selection case
# ---------------------------------------------------------------------------
def oracle_solver(X, r, opts, A0, B0, C0, *, device=-1, return_iters=True, observed=None, holdout=None,
                  patience=0):
    A, B, C, eh, k, info = hao.triple_decomp_ALS_holdout(X, observed, holdout, r, opts, A0, B0, C0, patience,
                                                         quiet)
    return A, B, C, eh, k, info


def test_the_oracle_picks_the_planted_rank_with_a_margin():
    """errHist on the fitted entries falls with r and would pick the largest
    rank; the held-out error picks the planted one, by at least 5 %."""
    from tritd import drivers
    c = hac.rank_selection_case()
    out = drivers.select_rank(c["X"], c["observed"], c["ranks"], c["holdout_ratio"], c["opts"], c["seed"],
                              factors=c["factors"], solver=oracle_solver)
    res = out["results"]
    print({r: (v["min_val"], v["best_iter"], v["errHist"][-1]) for r, v in res.items()})
    assert out["rank"] == c["planted"] == 3
    for r in c["ranks"]:
        if r != 3:
            assert res[3]["min_val"] <= 0.95 * res[r]["min_val"], r
    assert res[5]["errHist"][-1] < res[3]["errHist"][-1]
    H = out["holdout"]
    assert not (H & ~c["observed"]).any()
    assert H.sum() == int(np.floor(c["holdout_ratio"] * c["observed"].sum() + 0.5))
    np.testing.assert_array_equal(H, drivers.select_rank(c["X"], c["observed"], (), c["holdout_ratio"],
                                                         c["opts"], c["seed"])["holdout"])


# ---------------------------------------------------------------------------
# the new entry points, without a device
# ---------------------------------------------------------------------------
NEW = ("tritd_als_holdout_f64", "tritd_als_session_create_holdout", "tritd_als_session_holdout_info",
       "tritd_als_session_get_val", "tritd_als_session_get_best")


def test_new_symbols_are_bound_with_the_documented_signatures():
    import ctypes as C

    import tritd
    from tritd import _lib
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert _lib.SIGNATURES[name][0] is C.c_int
    # the masked forms' arguments plus `holdout` after observed and `patience` after opts
    ses = list(_lib.SIGNATURES["tritd_als_session_create_masked"][1])
    io = ses.index(C.POINTER(_lib.Opts))
    assert _lib.SIGNATURES["tritd_als_session_create_holdout"][1] == \
        ses[:4] + [vp] + ses[4:io + 1] + [i32] + ses[io + 1:]
    one = list(_lib.SIGNATURES["tritd_als_masked_f64"][1])
    io = one.index(C.POINTER(_lib.Opts))
    assert _lib.SIGNATURES["tritd_als_holdout_f64"][1] == \
        one[:2] + [vp] + one[2:io + 1] + [i32] + one[io + 1:-1] + [vp, vp, vp, vp, C.POINTER(i32),
                                                                  C.POINTER(i32)] + one[-1:]
    assert _lib.SIGNATURES["tritd_als_session_holdout_info"][1] == [vp, C.POINTER(i64), C.POINTER(C.c_double)]
    for f in (tritd.triple_decomp_ALS, tritd.AlsSession.__init__):
        p = inspect.signature(f).parameters
        assert p["holdout"].default is None and p["patience"].default == 0
    assert callable(tritd.AlsSession.get_best) and callable(tritd.AlsSession.holdout_info)
    assert inspect.signature(drivers_select_rank()).parameters["patience"].default == 0


def drivers_select_rank():
    from tritd import drivers
    return drivers.select_rank


def test_header_declares_the_new_entry_points_and_the_contract():
    import os

    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "tritd.h")).read()
    for name in NEW:
        assert ("tritd_status %s(" % name) in h
    for phrase in ("valHist(k)", "best_iter", "stop_reason", "patience"):
        assert phrase in h


def test_shape_mismatch_raises():
    import tritd
    g = hac.load("hals12x10x8_r2_stop")
    with pytest.raises(ValueError, match="holdout must have the shape of X"):
        tritd.triple_decomp_ALS(g["X"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"], observed=g["observed"],
                                holdout=g["holdout"][:, :, :-1])
    with pytest.raises(ValueError, match="holdout must have the shape of X"):
        tritd.AlsSession(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=12, n2=10, n3=8, X=g["X"],
                         holdout=g["holdout"].ravel())
    with pytest.raises(ValueError, match="observed must have the shape of X"):
        tritd.triple_decomp_ALS(g["X"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                observed=g["observed"][:-1], holdout=g["holdout"])
    with pytest.raises(ValueError, match=r"set_devices\(\[d\] \* P\)"):
        tritd.triple_decomp_ALS(g["X"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"], holdout=g["holdout"],
                                virtual_shards=2)
