"""Held-out validation of the masked ADMM: the oracle, the goldens and the
bindings, on the CPU (tests/holdout_admm_oracle.py, tests/holdout_admm_cases.py).
"""
import inspect
import os
import sys

import numpy as np
import pytest

import holdout_admm_cases as hc
import holdout_admm_oracle as ho
import masked_oracle as mo
from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_holdout_admm_golden as mk  # noqa: E402

SMALL = "hadm12x10x8_r2_p3"


def run(g, **kw):
    a = dict(D=g["D"], observed=g["observed"], holdout=g["holdout"], opts=g["opts"], patience=g["patience"],
             val_norm=g["val_norm"])
    a.update(kw)
    return ho.triple_decomp_ADMM_holdout(a["D"], a["observed"], a["holdout"], g["r"], a["opts"], g["A0"],
                                         g["B0"], g["C0"], a["patience"], a["val_norm"])


@pytest.fixture(scope="module")
def small():
    g = hc.load(SMALL)
    return g, run(g, patience=0)


# --- the oracle -----------------------------------------------------------------
def test_patience_zero_is_the_masked_oracle_bitwise(small):
    g, got = small
    A, B, C, O, eh, E, k, _ = mo.triple_decomp_ADMM_masked(g["D"], g["fit"], g["r"], g["opts"], g["A0"],
                                                           g["B0"], g["C0"])
    assert got["k"] == k == g["opts"]["maxIter"] and got["stop_reason"] == 0
    for key, ref in (("A", A), ("B", B), ("C", C), ("O", O), ("E", E), ("errHist", eh)):
        np.testing.assert_array_equal(got[key], ref)
    assert not got["O"][g["held_out"]].any() and not got["E"][g["held_out"]].any()
    assert np.any(got["E"])


def test_scores_are_those_of_the_returned_factors(small):
    """valHist(k), valHist1(k) score L_k of the factors after iteration k: the
    last entries from the returned A, B, C, entry best_iter from A_best, ..."""
    import tritd_oracle as orc
    g, got = small
    for it, f in ((got["k"], (got["A"], got["B"], got["C"])),
                  (got["best_iter"], (got["A_best"], got["B_best"], got["C_best"]))):
        v2, v1 = ho.scores(g["D"], g["held_out"], orc.triple_product(*f))
        assert (v2, v1) == (got["valHist"][it - 1], got["valHist1"][it - 1])
    best = mo.triple_decomp_ADMM_masked(g["D"], g["fit"], g["r"], dict(g["opts"], maxIter=got["best_iter"]),
                                        g["A0"], g["B0"], g["C0"])
    for key, ref in zip(("A_best", "B_best", "C_best"), best[:3]):
        np.testing.assert_array_equal(got[key], ref)


def test_a_flag_outside_omega_changes_nothing(small):
    g, ref = small
    miss = ~g["observed"]
    assert miss.any()
    D = g["D"].copy(order="F")
    D[miss] = np.nan
    got = run(g, D=D, holdout=g["holdout"] | miss, patience=0)
    for key in ("A", "B", "C", "O", "E", "errHist", "valHist", "valHist1"):
        np.testing.assert_array_equal(got[key], ref[key])
    assert (got["k"], got["best_iter"]) == (ref["k"], ref["best_iter"])


def test_val_norm_picks_the_history(small):
    g, ref = small
    other = run(g, patience=0, val_norm=3 - g["val_norm"])
    assert ref["best_iter"] == mk.first_argmin(ref["valHist1"]) != other["best_iter"] == \
        mk.first_argmin(ref["valHist"])
    np.testing.assert_array_equal(other["valHist"], ref["valHist"])


def test_patience_stops_like_a_reference_stop(small):
    g, free = small
    got = run(g)
    k, b = got["k"], got["best_iter"]
    assert got["stop_reason"] == 2 and 1 < b < k < g["opts"]["maxIter"] and k - b == g["patience"]
    for key in ("errHist", "valHist", "valHist1"):
        np.testing.assert_array_equal(got[key], free[key][:k])
    cut = mo.triple_decomp_ADMM_masked(g["D"], g["fit"], g["r"], dict(g["opts"], maxIter=k), g["A0"], g["B0"],
                                       g["C0"])
    for key, ref in zip(("A", "B", "C", "O"), cut[:4]):
        np.testing.assert_array_equal(got[key], ref)


def test_oracle_refusals(small):
    g, _ = small
    D0 = g["D"].copy(order="F")
    D0[g["held_out"]] = 0.0
    for kw in (dict(holdout=None), dict(holdout=np.zeros(g["D"].shape, dtype=bool)),
               dict(holdout=~g["observed"]), dict(holdout=np.ones(g["D"].shape, dtype=bool)), dict(D=D0),
               dict(patience=-1), dict(val_norm=0), dict(val_norm=3)):
        with pytest.raises(ValueError):
            run(g, **kw)


# --- the goldens ------------------------------------------------------------------
def test_the_goldens_cover_what_the_issue_lists():
    gs = {n: hc.load(n) for n in hc.names()}
    assert sorted((g["D"].shape, g["r"]) for g in gs.values()) == sorted([
        ((12, 10, 8), 2), ((30, 30, 30), 3), ((20, 6, 70), 3), ((17, 16, 20), 8), ((24, 20, 18), 12),
        ((24, 22, 20), 16)])
    assert any(g["stop_reason"] == 2 and 1 < g["best_iter"] < g["k"] for g in gs.values())
    assert any(g["stop_reason"] == 1 and g["k"] < g["opts"]["maxIter"] for g in gs.values())
    assert any(g["val_norm"] == 1 and g["best_iter"] != g["best_iter_other"] for g in gs.values())
    assert sum(g["stop_reason"] == 0 and g["k"] == g["opts"]["maxIter"] for g in gs.values()) >= 3
    t = gs["hadm30_r3_tiles"]
    assert t["held_out"][:16, 0, :16].all() and not t["held_out"][:16, 1, :16].any()
    assert (t["holdout"] & ~t["observed"]).any()
    for g in gs.values():
        assert g["opts"]["lambda"] == mk.active_lambda(g["D"])
        assert os.path.getsize(os.path.join(GOLDEN, g["name"] + ".npz")) < (1 << 20)


@pytest.mark.parametrize("name", hc.names())
def test_golden_reloads_and_passes_admission(name):
    g = hc.load(name)
    assert mk.admitted(g) == []
    for key, tol in hc.DRIFTS.items():
        assert float(g["drift_" + key]) * hc.MARGIN <= tol, key
    hist = g["valHist1"] if g["val_norm"] == 1 else g["valHist"]
    for m in (hc.decision_margins(hist), hc.stop_margins(g["errHist"], g["opts"]["tol"])):
        assert m.size == 0 or m.min() >= hc.DECISION_MARGIN
    got = run(g)
    for key in ("k", "best_iter", "stop_reason"):
        assert got[key] == g[key], key
    for key in ("A", "B", "C", "O", "E", "errHist", "valHist", "valHist1", "A_best", "B_best", "C_best"):
        np.testing.assert_array_equal(got[key], g[key], err_msg=key)
    d, observed, H, r, opts, patience, val_norm = mk.case_inputs(name)
    np.testing.assert_array_equal(d["D"], g["D"])
    np.testing.assert_array_equal(H, g["holdout"])
    assert (opts, patience, val_norm) == (g["opts"], g["patience"], g["val_norm"])


def test_sweep_holdout_reaches_the_tile_cases():
    import masked_sweep_cases as ms
    for r in ms.SCHEDULE_RANKS:
        W, H = ms.mask(("cp", r)), hc.sweep_holdout(("cp", r))
        assert (H & W)[:16, 3, :16].all() and not (H & W)[:16, 4, :16].any()
        assert H[:16, 1, 16:32].all() and not W[:16, 1, 16:32].any()
        assert (W & ~H).any() and 0.09 < (H & W).sum() / W.sum() < 0.13


# --- the new entry points, without a device -------------------------------------------
NEW = ("tritd_admm_holdout_f64", "tritd_session_create_holdout", "tritd_session_holdout_info",
       "tritd_session_get_val", "tritd_session_get_best", "tritd_session_holdout_ms")


def test_new_symbols_are_bound_with_the_documented_signatures():
    import ctypes as C

    import tritd
    from tritd import _lib, drivers
    vp, i32, i64, dp = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert _lib.SIGNATURES[name][0] is C.c_int
    # the masked forms' arguments plus `holdout` after observed, `patience, val_norm` after opts
    ses = list(_lib.SIGNATURES["tritd_session_create_masked"][1])
    io = ses.index(C.POINTER(_lib.Opts))
    assert _lib.SIGNATURES["tritd_session_create_holdout"][1] == \
        ses[:4] + [vp] + ses[4:io + 1] + [i32, i32] + ses[io + 1:]
    one = list(_lib.SIGNATURES["tritd_admm_masked_f64"][1])
    io = one.index(C.POINTER(_lib.Opts))
    assert _lib.SIGNATURES["tritd_admm_holdout_f64"][1] == \
        one[:2] + [vp] + one[2:io + 1] + [i32, i32] + one[io + 1:-1] + \
        [vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)] + one[-1:]
    assert _lib.SIGNATURES["tritd_session_holdout_info"][1] == [vp, C.POINTER(i64), dp, dp]
    for f in (tritd.triple_decomp_ADMM, tritd.Session.__init__):
        p = inspect.signature(f).parameters
        assert p["holdout"].default is None and p["patience"].default == 0 and p["val_norm"].default == 2
    for m in ("get_best", "get_val", "holdout_info"):
        assert callable(getattr(tritd.Session, m))
    p = inspect.signature(drivers.select_rank).parameters
    assert p["solver"].kind is p["lambdas"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["solver"].default is None and p["lambdas"].default is None


def test_header_declares_the_new_entry_points_and_the_contract():
    h = open(os.path.join(ROOT, "include", "tritd.h")).read()
    for name in NEW:
        assert ("tritd_status %s(" % name) in h
    for phrase in ("valHist(k)", "valHist1(k)", "best_iter", "stop_reason", "patience", "val_norm",
                   "NOT kept", "TRITD_MODEL_QI"):
        assert phrase in h


def test_python_argument_checks(small):
    import tritd
    from tritd import drivers
    g, _ = small
    a = (g["D"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"])
    with pytest.raises(ValueError, match="holdout must have the shape of D"):
        tritd.triple_decomp_ADMM(*a, observed=g["observed"], holdout=g["holdout"][:, :, :-1])
    with pytest.raises(ValueError, match="holdout must have the shape of D"):
        tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=12, n2=10, n3=8, D=g["D"],
                      holdout=g["holdout"].ravel())
    with pytest.raises(ValueError, match="observed must have the shape of D"):
        tritd.triple_decomp_ADMM(*a, observed=g["observed"][:-1], holdout=g["holdout"])
    with pytest.raises(ValueError, match=r"set_devices\(\[d\] \* P\)"):
        tritd.triple_decomp_ADMM(*a, holdout=g["holdout"], virtual_shards=2)
    with pytest.raises(tritd.TritdError) as e:
        tritd.triple_decomp_ADMM(g["D"].astype(np.float32), *a[1:], holdout=g["holdout"])
    assert e.value.status == tritd._lib.TRITD_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="solver must be"):
        drivers.select_rank(g["D"], g["observed"], (2,), solver="sgd")
    with pytest.raises(ValueError, match="needs the ADMM opts"):
        drivers.select_rank(g["D"], g["observed"], (2,), solver="admm")


def test_the_oracle_picks_the_planted_rank_where_errhist_does_not():
    from tritd import drivers
    c = hc.rank_selection_case()
    H = drivers.holdout_mask(c["observed"], c["holdout_ratio"], np.random.default_rng(c["seed"]))
    res = {}
    for r in c["ranks"]:
        for lam in c["lambdas"]:
            o = dict(c["opts"])
            o["lambda"] = lam
            q = ho.triple_decomp_ADMM_holdout(c["X"], c["observed"], H, r, o, *c["factors"](r))
            res[(r, lam)] = (q["valHist"][q["best_iter"] - 1], q["errHist"][-1])
    print(res)
    by_val = min(res, key=lambda key: res[key][0])
    assert by_val == (c["planted"], c["lambdas"][1]) == (3, c["lambdas"][1])
    for key, v in res.items():  # by a factor of 3 at least
        assert key == by_val or v[0] >= 3.0 * res[by_val][0]
    assert min(res, key=lambda key: res[key][1])[0] != c["planted"]
