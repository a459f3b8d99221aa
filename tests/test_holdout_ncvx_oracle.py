"""Held-out validation of the masked nonconvex solver: the oracle, the goldens
and the bindings, on the CPU (tests/holdout_ncvx_oracle.py,
tests/holdout_ncvx_cases.py).
"""
import inspect
import os
import sys

import numpy as np
import pytest

import holdout_ncvx_cases as hc
import holdout_ncvx_oracle as hno
import masked_ncvx_oracle as mno
from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_holdout_ncvx_golden as mk  # noqa: E402

SMALL = "hnc12x10x8_r2_p"


def run(g, **kw):
    a = dict(X=g["X"], observed=g["observed"], holdout=g["holdout"], patience=g["patience"],
             val_norm=g["val_norm"], over={})
    a.update(kw)
    return hno.triple_decomp_ncvx_holdout(a["X"], a["observed"], a["holdout"], g["r"],
                                          *hc.args(g, **a["over"]), g["A0"], g["B0"], g["C0"],
                                          a["patience"], a["val_norm"])


def masked(g, **over):
    return mno.triple_decomp_ncvx_masked(g["X"], g["fit"], g["r"], *hc.args(g, **over), g["A0"], g["B0"],
                                         g["C0"], printer=hno.quiet)


@pytest.fixture(scope="module")
def small():
    g = hc.load(SMALL)
    return g, run(g, patience=0)


# --- the oracle -----------------------------------------------------------------
def test_patience_zero_is_the_masked_oracle_bitwise(small):
    g, got = small
    A, B, C, O, eh, k, _ = masked(g)
    assert got["k"] == k == g["opts"]["maxIter"] and got["stop_reason"] == 0
    for key, ref in (("A", A), ("B", B), ("C", C), ("O", O), ("errHist", eh)):
        np.testing.assert_array_equal(got[key], ref)
    assert not got["O"][~g["fit"]].any()
    assert 0 < np.count_nonzero(got["O"][g["fit"]]) < g["fit"].sum()


def test_scores_are_those_of_the_factors_the_iteration_started_with(small):
    """valHist(k), valHist1(k) score T_k of :35: entry 1 from A0, B0, C0, entry
    k from a masked run of k - 1 iterations, entry best_iter from A_best, ..."""
    import tritd_oracle as orc
    g, got = small
    n1, n2, n3 = g["X"].shape
    r = g["r"]
    f0 = (g["A0"].reshape((n1, r, r), order="F"), g["B0"].reshape((r, n2, r), order="F"),
          g["C0"].reshape((r, r, n3), order="F"))
    prev = masked(g, maxIter=got["k"] - 1)[:3]
    best = masked(g, maxIter=got["best_iter"] - 1)[:3]
    assert got["best_iter"] > 1
    for key, ref in zip(("A_best", "B_best", "C_best"), best):
        np.testing.assert_array_equal(got[key], ref)
    for it, f in ((1, f0), (got["k"], prev), (got["best_iter"], best)):
        v2, v1 = hno.scores(g["X"], g["held_out"], orc.triple_product(*f))
        assert (v2, v1) == (got["valHist"][it - 1], got["valHist1"][it - 1])
    # k = 1 always taken: one iteration keeps A0, B0, C0 exactly
    one = run(g, patience=0, over=dict(maxIter=1))
    assert one["best_iter"] == 1
    for key, ref in zip(("A_best", "B_best", "C_best"), f0):
        np.testing.assert_array_equal(one[key], ref)


def test_a_flag_outside_omega_changes_nothing(small):
    g, ref = small
    miss = ~g["observed"]
    assert miss.any()
    X = g["X"].copy(order="F")
    X[miss] = np.nan
    got = run(g, X=X, holdout=g["holdout"] | miss, patience=0)
    for key in ("A", "B", "C", "O", "errHist", "valHist", "valHist1"):
        np.testing.assert_array_equal(got[key], ref[key])
    assert (got["k"], got["best_iter"]) == (ref["k"], ref["best_iter"])


def test_val_norm_picks_the_history(small):
    g, ref = small
    other = run(g, patience=0, val_norm=3 - g["val_norm"])
    assert g["val_norm"] == 2
    assert ref["best_iter"] == mk.first_argmin(ref["valHist"]) != other["best_iter"] == \
        mk.first_argmin(ref["valHist1"])
    for key in ("valHist", "valHist1", "errHist", "A"):
        np.testing.assert_array_equal(other[key], ref[key])


def test_patience_stops_like_a_reference_break(small):
    g, free = small
    got = run(g)
    k, b = got["k"], got["best_iter"]
    assert got["stop_reason"] == 2 and 1 < b < k < g["opts"]["maxIter"] and k - b == g["patience"]
    for key in ("errHist", "valHist", "valHist1"):
        np.testing.assert_array_equal(got[key], free[key][:k])
    # the updates of k have run; O is that of k-1 (:67 before :71)
    cut = masked(g, maxIter=k)
    for key, ref in zip(("A", "B", "C"), cut[:3]):
        np.testing.assert_array_equal(got[key], ref)
    np.testing.assert_array_equal(got["O"], masked(g, maxIter=k - 1)[3])
    assert np.any(got["O"] != cut[3])


def test_lambda_moves_o_and_leaves_the_scores(small):
    """The factor updates :49-51 read X, not Y: lambda is no axis of a
    validation grid for this solver."""
    g, ref = small
    other = run(g, patience=0, over={"lambda": 0.05})
    for key in ("valHist", "valHist1", "A", "B", "C"):
        np.testing.assert_array_equal(other[key], ref[key])
    assert np.any(other["O"] != ref["O"]) and np.any(other["errHist"] != ref["errHist"])


def test_oracle_refusals(small):
    g, _ = small
    X0 = g["X"].copy(order="F")
    X0[g["held_out"]] = 0.0
    for kw in (dict(holdout=None), dict(holdout=np.zeros(g["X"].shape, dtype=bool)),
               dict(holdout=~g["observed"]), dict(holdout=np.ones(g["X"].shape, dtype=bool)), dict(X=X0),
               dict(patience=-1), dict(val_norm=0), dict(val_norm=3), dict(over=dict(rho=0.0))):
        with pytest.raises(ValueError):
            run(g, **kw)


# --- the goldens ------------------------------------------------------------------
def test_the_goldens_cover_what_the_issue_lists():
    gs = {n: hc.load(n) for n in hc.names()}
    assert sorted((g["X"].shape, g["r"]) for g in gs.values()) == sorted([
        ((12, 10, 8), 2), ((21, 13, 35), 5), ((18, 19, 22), 6), ((17, 16, 20), 8), ((20, 6, 70), 3),
        ((30, 30, 30), 3)])
    assert {hc.padded_rank(g["r"]) for g in gs.values()} == {16, 32, 48, 64}
    assert sum(g["stop_reason"] == 2 and 1 < g["best_iter"] < g["k"] for g in gs.values()) == 1
    assert sum(g["stop_reason"] == 1 and g["k"] < g["opts"]["maxIter"] for g in gs.values()) == 1
    assert sum(g["stop_reason"] == 0 and g["k"] == g["opts"]["maxIter"] for g in gs.values()) == 4
    assert any(g["val_norm"] == 1 for g in gs.values())
    t = gs["hnc30_r3_tiles"]
    assert t["held_out"][:16, 0, :16].all() and not t["held_out"][:16, 1, :16].any()
    assert (t["holdout"] & ~t["observed"]).any()
    for g in gs.values():
        assert {k: g["opts"][k] for k in mk.NCVX_PARAMS} == mk.NCVX_PARAMS
        assert os.path.getsize(os.path.join(GOLDEN, g["name"] + ".npz")) < (1 << 20)


@pytest.mark.parametrize("name", hc.names())
def test_golden_reloads_and_passes_admission(name):
    g = hc.load(name)
    assert mk.admitted(g) == []
    nz = np.count_nonzero(g["O"][g["fit"]])
    assert 0 < nz < g["fit"].sum() and not g["O"][~g["fit"]].any()
    assert np.all(np.isfinite(g["valHist"])) and np.all(np.isfinite(g["valHist1"]))
    for key, tol in hc.DRIFTS.items():
        assert float(g["drift_" + key]) * hc.MARGIN <= tol, key
    hist = g["valHist1"] if g["val_norm"] == 1 else g["valHist"]
    for m in (hc.decision_margins(hist), hc.stop_margins(g["errHist"], g["opts"]["tol"])):
        assert m.size == 0 or m.min() >= hc.DECISION_MARGIN
    got = run(g)
    for key in ("k", "best_iter", "stop_reason"):
        assert got[key] == g[key], key
    for key in ("A", "B", "C", "O", "errHist", "valHist", "valHist1", "A_best", "B_best", "C_best"):
        np.testing.assert_array_equal(got[key], g[key], err_msg=key)
    d, observed, H, r, prm, patience, val_norm = mk.case_inputs(name)
    np.testing.assert_array_equal(d["X"], g["X"])
    np.testing.assert_array_equal(H, g["holdout"])
    assert (prm, patience, val_norm) == (g["opts"], g["patience"], g["val_norm"])


# --- the new entry points, without a device -------------------------------------------
NEW = ("tritd_ncvx_holdout_f64", "tritd_als_session_create_ncvx_holdout", "tritd_als_session_get_val2",
       "tritd_als_session_holdout_ms")


def test_new_symbols_are_bound_with_the_documented_signatures():
    import ctypes as C

    import tritd
    from tritd import _lib, drivers
    vp, i32, dp = C.c_void_p, C.c_int32, C.POINTER(C.c_double)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert _lib.SIGNATURES[name][0] is C.c_int
    # the masked call's arguments plus `holdout` after observed, `patience, val_norm` after tol,
    # and the seven holdout outputs before device
    one = list(_lib.SIGNATURES["tritd_ncvx_masked_f64"][1])
    it = one.index(C.c_double) + 7   # rho .. theta, maxIter, then tol
    assert one[it] is C.c_double and one[it - 1] is i32
    assert _lib.SIGNATURES["tritd_ncvx_holdout_f64"][1] == \
        one[:2] + [vp] + one[2:it + 1] + [i32, i32] + one[it + 1:-1] + \
        [vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)] + one[-1:]
    # the ALS holdout creator's arguments plus val_norm and the six parameters after patience
    ses = list(_lib.SIGNATURES["tritd_als_session_create_holdout"][1])
    io = ses.index(C.POINTER(_lib.Opts))
    assert _lib.SIGNATURES["tritd_als_session_create_ncvx_holdout"][1] == \
        ses[:io + 2] + [i32] + [C.c_double] * 6 + ses[io + 2:]
    assert _lib.SIGNATURES["tritd_als_session_get_val2"][1] == [vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    assert _lib.SIGNATURES["tritd_als_session_holdout_ms"][1] == [vp, dp, dp]
    for f in (tritd.triple_decomp_ncvx, tritd.NcvxSession.__init__):
        p = inspect.signature(f).parameters
        assert p["patience"].default == 0 and p["val_norm"].default == 2
    assert inspect.signature(tritd.triple_decomp_ncvx).parameters["holdout"].default is None
    assert issubclass(tritd.NcvxSession, tritd.AlsSession)
    for m in ("run", "sync", "get", "get_O", "get_best", "get_val", "holdout_info", "holdout_ms"):
        assert callable(getattr(tritd.NcvxSession, m))
    p = inspect.signature(drivers.select_rank).parameters
    assert p["gammas"].kind is inspect.Parameter.KEYWORD_ONLY and p["gammas"].default is None


def test_header_declares_the_new_entry_points_and_the_contract():
    h = open(os.path.join(ROOT, "include", "tritd.h")).read()
    for name in NEW:
        assert ("tritd_status %s(" % name) in h
    for phrase in ("valHist1(k) = sum_{H & Omega} |X - T_k|", "O is that of k-1 (:71)",
                   "val_norm not 1 or 2", "tritd_als_session_create_ncvx_holdout",
                   "tritd_als_session_set_ncvx on such a session is TRITD_ERR_UNSUPPORTED"):
        assert phrase in h, phrase


def test_python_argument_checks(small):
    import tritd
    from tritd import drivers
    g, _ = small
    a = (g["X"], g["r"], *hc.args(g), g["A0"], g["B0"], g["C0"])
    with pytest.raises(ValueError, match="holdout must have the shape of X"):
        tritd.triple_decomp_ncvx(*a, observed=g["observed"], holdout=g["holdout"][:, :, :-1])
    with pytest.raises(ValueError, match="observed must have the shape of X"):
        tritd.triple_decomp_ncvx(*a, observed=g["observed"][:-1], holdout=g["holdout"])
    with pytest.raises(ValueError, match="need holdout"):
        tritd.triple_decomp_ncvx(*a, observed=g["observed"], patience=2)
    with pytest.raises(ValueError, match="need holdout"):
        tritd.triple_decomp_ADMM_outlier(*a, val_norm=1)
    kw = dict(n1=12, n2=10, n3=8, X=g["X"], ncvx=hc.ncvx_dict(hc.args(g)))
    o = dict(maxIter=5, tol=0.0)
    with pytest.raises(ValueError, match="NcvxSession needs holdout"):
        tritd.NcvxSession(g["r"], o, g["A0"], g["B0"], g["C0"], holdout=None, **kw)
    with pytest.raises(ValueError, match="holdout must have the shape of X"):
        tritd.NcvxSession(g["r"], o, g["A0"], g["B0"], g["C0"], holdout=g["holdout"].ravel(), **kw)
    with pytest.raises(ValueError, match="solver must be"):
        drivers.select_rank(g["X"], g["observed"], (2,), solver="sgd")
    with pytest.raises(ValueError, match="needs the nonconvex parameters"):
        drivers.select_rank(g["X"], g["observed"], (2,), solver="ncvx")
    with pytest.raises(ValueError, match="opts lacks gamma_A, theta"):
        drivers.select_rank(g["X"], g["observed"], (2,), solver="ncvx",
                            opts=dict(rho=1.0, lam=0.5, epsilon=1e-2, p=0.5, maxIter=3, tol=0.0))


def test_the_oracle_picks_the_planted_rank_where_errhist_does_not():
    from tritd import drivers
    c = hc.rank_selection_case()
    H = drivers.holdout_mask(c["observed"], c["holdout_ratio"], np.random.default_rng(c["seed"]))
    o = c["opts"]
    res = {}
    for r in c["ranks"]:
        for gam in c["gammas"]:
            q = hno.triple_decomp_ncvx_holdout(c["X"], c["observed"], H, r, o["rho"], o["lam"], gam,
                                               o["epsilon"], o["p"], o["theta"], o["maxIter"], o["tol"],
                                               *c["factors"](r))
            res[(r, gam)] = (q["valHist"][q["best_iter"] - 1], q["errHist"][-1])
    print(res)
    by_val = min(res, key=lambda key: res[key][0])
    assert by_val == (c["planted"], c["gammas"][0]) == (3, 1e-3)
    for key, v in res.items():
        # every other rank or gamma_A scores at least 10 % worse; rank 2 cannot
        # represent the planted tensor: 3x at the very least
        assert key == by_val or v[0] >= (3.0 if key[0] == 2 else 1.1) * res[by_val][0]
    assert min(res, key=lambda key: res[key][1])[0] != c["planted"]
