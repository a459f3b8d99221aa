"""Held-out validation of the masked ADMM on the GPU (holdout=, patience=,
val_norm=; include/tritd.h: tritd_admm_holdout_f64).

Reference: tests/holdout_admm_oracle.py through the goldens of
tests/holdout_admm_cases.py, at the tolerances of tests/masked_cases.py (L, O, E
<= 1e-9; A, B, C <= 1e-8; errHist, valHist, valHist1 within 1e-8 |ref| + 1e-11;
the same k, best_iter and stop_reason), and the masked call itself
(triple_decomp_ADMM(observed = Omega & ~H)), bit for bit.
"""
import numpy as np
import pytest

import holdout_admm_cases as hc
import masked_sweep_cases as ms

pytestmark = pytest.mark.gpu

FIT_KEYS = ("A", "B", "C", "O", "E", "errHist")
CP_SCHEDULE = [("cp", r) for r in ms.SCHEDULE_RANKS]
CP_NARROW = [("cp", r) for r in ms.NARROW]


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


def rel(a, b):
    den = np.linalg.norm(np.ravel(b))
    return float(np.linalg.norm(np.ravel(a - b)) / (den if den > 0 else 1.0))


def gate(a, b):
    return float(np.max(np.abs(a - b) / (hc.TOL_ERR * np.abs(b) + hc.ATOL_ERR)))


def solve(tritd, g, **kw):
    """dict(A, B, C, O, E, errHist, k, + the holdout dict) of the one-shot call."""
    a = dict(observed=g["observed"], holdout=g["holdout"], patience=g.get("patience", 0),
             val_norm=g.get("val_norm", 2), opts=g["opts"], D=g["D"])
    a.update(kw)
    D, opts = a.pop("D"), a.pop("opts")
    A, B, C, O, eh, E, k, v = tritd.triple_decomp_ADMM(D, g["r"], opts, g["A0"], g["B0"], g["C0"],
                                                       return_E=True, return_iters=True, **a)
    return dict(v, A=A, B=B, C=C, O=O, E=E, errHist=eh, k=k)


def solve_masked(tritd, g, observed, **kw):
    A, B, C, O, eh, E, k = tritd.triple_decomp_ADMM(kw.pop("D", g["D"]), g["r"], kw.pop("opts", g["opts"]),
                                                    g["A0"], g["B0"], g["C0"], return_E=True,
                                                    return_iters=True, observed=observed, **kw)
    return dict(A=A, B=B, C=C, O=O, E=E, errHist=eh, k=k)


def session(tritd, g, comm=None, **kw):
    n1, n2, n3 = g["D"].shape
    a = dict(D=g["D"], observed=g["observed"], holdout=g["holdout"], patience=g.get("patience", 0),
             val_norm=g.get("val_norm", 2), opts=g["opts"])
    a.update(kw)
    return tritd.Session(g["r"], a.pop("opts"), g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3, device=0,
                         comm=comm, probe=False, **a)


def session_result(s):
    x = s.get()
    b = s.get_best()
    return dict(x, A_best=b["A"], B_best=b["B"], C_best=b["C"])


def same(got, ref, keys):
    for key in keys:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


def check(orc, got, g, what=""):
    """Every figure printed before it is asserted."""
    fig = dict(k=got["k"], best=got["best_iter"], stop=got["stop_reason"],
               L=rel(orc.triple_product(got["A"], got["B"], got["C"]),
                     orc.triple_product(g["A"], g["B"], g["C"])),
               O=rel(got["O"], g["O"]), E=rel(got["E"], g["E"]))
    for key in ("A", "B", "C", "A_best", "B_best", "C_best"):
        fig[key] = rel(got[key], g[key])
    n = {key: min(len(got[key]), len(g[key])) for key in ("errHist", "valHist", "valHist1")}
    for key in n:
        fig[key] = gate(got[key][:n[key]], g[key][:n[key]])
    print(g["name"], what, " ".join("%s=%.2e" % kv for kv in fig.items()), flush=True)
    assert (got["k"], got["best_iter"], got["stop_reason"]) == (g["k"], g["best_iter"], g["stop_reason"])
    for key in n:
        assert len(got[key]) == g["k"]
        np.testing.assert_allclose(got[key], g[key], rtol=hc.TOL_ERR, atol=hc.ATOL_ERR, err_msg=key)
    for key in ("L", "O", "E"):
        assert fig[key] <= hc.TOL_LOE, key
    for key in ("A", "B", "C", "A_best", "B_best", "C_best"):
        assert fig[key] <= hc.TOL_ABC, key
    out = ~g["fit"]  # held out or unobserved
    assert not got["O"][out].any() and not got["E"][out].any()
    assert got["holdout_count"] == int(g["held_out"].sum())


def sweep_case(case):
    g = ms.inputs(case)
    g["holdout"] = hc.sweep_holdout(case)
    g["fit"] = g["observed"] & ~g["holdout"]
    g["held_out"] = g["observed"] & g["holdout"]
    return g


def ids(cases):
    return [ms.case_id(c) for c in cases]


# --- 1. the goldens ---------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.names())
def test_holdout_admm_matches_golden(tritd, orc, name):
    g = hc.load(name)
    check(orc, solve(tritd, g), g, "one-shot")


# --- 2. patience = 0 is the masked call, bit for bit ----------------------------------------
def bitwise_against_masked(tritd, orc, case, what):
    g = sweep_case(case)
    got = solve(tritd, g)
    ref = solve_masked(tritd, g, g["fit"])
    assert np.any(ref["E"]) and got["k"] == ref["k"] == ms.ITERS and got["stop_reason"] == 0
    same(got, ref, FIT_KEYS)
    assert not got["O"][g["held_out"]].any() and not got["E"][g["held_out"]].any()
    # the scores against the host's, from the returned factors (the last entry)
    # and from the best iterate (entry best_iter)
    x = g["D"][g["held_out"]]
    fig = {}
    for it, f in ((got["k"], ("A", "B", "C")), (got["best_iter"], ("A_best", "B_best", "C_best"))):
        d = x - orc.triple_product(*(got[key] for key in f))[g["held_out"]]
        v2, v1 = np.linalg.norm(d) / np.linalg.norm(x), np.abs(d).sum() / np.abs(x).sum()
        fig[it] = (gate(got["valHist"][it - 1:it], np.array([v2])),
                   gate(got["valHist1"][it - 1:it], np.array([v1])))
    print("  holdout sweep %s %s best=%d scores (gate units) %s" % (ms.case_id(case), what, got["best_iter"], fig),
          flush=True)
    assert all(max(v) <= 1.0 for v in fig.values())
    assert got["best_iter"] == 1 + int(np.argmin(got["valHist"]))


@pytest.mark.parametrize("case", CP_SCHEDULE, ids=ids(CP_SCHEDULE))
def test_bitwise_compact_e(tritd, orc, case):
    bitwise_against_masked(tritd, orc, case, "default")


@pytest.mark.parametrize("case", CP_NARROW, ids=ids(CP_NARROW))
def test_bitwise_dense_e(tritd, orc, case, monkeypatch):
    monkeypatch.setenv("TRITD_DENSE_E", "1")
    bitwise_against_masked(tritd, orc, case, "TRITD_DENSE_E=1")


@pytest.mark.parametrize("case", CP_SCHEDULE, ids=ids(CP_SCHEDULE))
def test_bitwise_split_t_walk(tritd, orc, case, monkeypatch):
    monkeypatch.setenv("TRITD_K5_TSPLIT", "2")
    bitwise_against_masked(tritd, orc, case, "TRITD_K5_TSPLIT=2")


@pytest.mark.parametrize("case", CP_NARROW, ids=ids(CP_NARROW))
def test_bitwise_side_stream_schedule(tritd, orc, case, monkeypatch):
    monkeypatch.setenv("TRITD_FUSED", "0")
    bitwise_against_masked(tritd, orc, case, "TRITD_FUSED=0")


# --- 3. the scores step by step, the best iterate ----------------------------------------------
def test_scores_against_the_host_after_each_single_step(tritd, orc):
    g = hc.load("hadm20x6x70_r3_l1")
    x = g["D"][g["held_out"]]
    s = session(tritd, g)
    try:
        cnt, nrm, s1 = s.holdout_info()
        assert cnt == int(g["held_out"].sum())
        assert abs(nrm - np.linalg.norm(x)) <= 1e-13 * nrm and abs(s1 - np.abs(x).sum()) <= 1e-13 * s1
        assert s.mask_info() == (True, int(g["fit"].sum()))
        assert s.get_val()["best_iter"] == 0
        same(s.get_best(), dict(A=g["A0"], B=g["B0"], C=g["C0"]), "ABC")
        worst = 0.0
        for k in range(1, 9):
            s.run(1)
            r = s.get()
            assert r["k"] == k and len(r["valHist"]) == len(r["valHist1"]) == k
            d = x - orc.triple_product(r["A"], r["B"], r["C"])[g["held_out"]]
            v2, v1 = np.linalg.norm(d) / np.linalg.norm(x), np.abs(d).sum() / np.abs(x).sum()
            worst = max(worst, gate(r["valHist"][-1:], np.array([v2])), gate(r["valHist1"][-1:], np.array([v1])))
            np.testing.assert_allclose(r["valHist"], g["valHist"][:k], rtol=hc.TOL_ERR, atol=hc.ATOL_ERR)
            np.testing.assert_allclose(r["valHist1"], g["valHist1"][:k], rtol=hc.TOL_ERR, atol=hc.ATOL_ERR)
        print("  scores against the host, worst of 8 steps: %.2e of the gate" % worst, flush=True)
        assert worst <= 1.0
    finally:
        s.close()


@pytest.mark.parametrize("name", ["hadm12x10x8_r2_p3", "hadm17x16x20_r8_stop"])
def test_get_best_is_the_masked_run_to_best_iter_bitwise(tritd, name):
    g = hc.load(name)
    got = solve(tritd, g)
    assert got["best_iter"] == g["best_iter"]
    ref = solve_masked(tritd, g, g["fit"], opts=dict(g["opts"], maxIter=g["best_iter"], tol=0.0))
    assert ref["k"] == g["best_iter"]
    for key in "ABC":
        np.testing.assert_array_equal(got[key + "_best"], ref[key])
    # and the outputs of a patience / :63 stop are those of the masked run to k
    cut = solve_masked(tritd, g, g["fit"], opts=dict(g["opts"], maxIter=g["k"]))
    same(got, cut, FIT_KEYS)


# --- 4. fill values, sessions -----------------------------------------------------------------------
def test_nan_and_inf_at_flags_outside_omega(tritd):
    g = hc.load("hadm30_r3_tiles")
    ref = solve(tritd, g)
    miss = ~g["observed"]
    assert (g["holdout"] & miss).any()
    for fill in (np.nan, np.inf):
        D = g["D"].copy(order="F")
        D[miss] = fill
        got = solve(tritd, g, D=D, holdout=g["holdout"] | miss)
        same(got, ref, FIT_KEYS + ("valHist", "valHist1", "A_best", "B_best", "C_best"))
        assert (got["k"], got["best_iter"], got["holdout_count"]) == (ref["k"], ref["best_iter"],
                                                                      int(g["held_out"].sum()))


ALL_KEYS = FIT_KEYS + ("valHist", "valHist1", "A_best", "B_best", "C_best")


def test_session_stepped_3_plus_7_against_10(tritd):
    g = sweep_case(("cp", 6))
    whole = solve(tritd, g)
    s = session(tritd, g)
    try:
        s.run(3)
        s.run(7)
        got = session_result(s)
    finally:
        s.close()
    same(got, whole, ALL_KEYS)
    assert (got["k"], got["best_iter"], got["stop_reason"]) == (10, whole["best_iter"], 0)


def test_a_run_after_a_patience_stop_is_a_no_op(tritd, orc):
    g = hc.load("hadm12x10x8_r2_p3")
    s = session(tritd, g)
    try:
        s.run(g["opts"]["maxIter"])
        got = session_result(s)
        assert s.sync() == (g["k"], True)
        s.run(3)
        again = session_result(s)
    finally:
        s.close()
    check(orc, dict(got, holdout_count=int(g["held_out"].sum())), g, "session")
    same(again, got, ALL_KEYS)
    assert (again["k"], again["best_iter"], again["stop_reason"]) == (got["k"], got["best_iter"], 2)


def test_session_with_device_masks_and_padded_leading_dimension(tritd):
    """D and both masks resident on the device, ldD = n1 + 5 (elements of D,
    bytes of the masks), the padding rows holding NaN / nonzero bytes."""
    from tritd import hip
    g = sweep_case(("cp", 11))
    whole = solve(tritd, g)
    n1, n2, n3 = g["D"].shape
    ld = n1 + 5
    Dp = np.full((ld, n2, n3), np.nan, order="F")
    Dp[:n1] = g["D"]
    Mp = np.full((ld, n2, n3), 0xFF, dtype=np.uint8, order="F")
    Mp[:n1] = g["observed"]
    Hp = np.full((ld, n2, n3), 0xFF, dtype=np.uint8, order="F")
    Hp[:n1] = g["holdout"]
    dev = [hip.DeviceArray.from_host(x) for x in (Dp, Mp, Hp)]
    try:
        s = session(tritd, g, D=None, d_device_ptr=dev[0].ptr, ldD=ld, observed=dev[1].ptr, holdout=dev[2].ptr)
    finally:
        for d in dev:
            d.free()
    try:
        assert s.holdout_info()[0] == int(g["held_out"].sum())
        assert s.mask_info() == (True, int(g["fit"].sum()))
        s.run(ms.ITERS)
        got = session_result(s)
    finally:
        s.close()
    same(got, whole, ALL_KEYS)
    assert got["best_iter"] == whole["best_iter"]


# --- 5. shards ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shov", ["1", "0"])
@pytest.mark.parametrize("name", ["hadm30_r3_tiles", "hadm12x10x8_r2_p3", "hadm24x20x18_r12"])
def test_device_set_matches_golden(tritd, orc, name, shov, monkeypatch):
    monkeypatch.setenv("TRITD_SHOV", shov)
    g = hc.load(name)
    tritd.set_devices([0, 0, 0])
    try:
        got = solve(tritd, g)
    finally:
        tritd.set_devices([])
    check(orc, got, g, "set_devices([0,0,0]) TRITD_SHOV=" + shov)


@pytest.mark.parametrize("shov", ["1", "0"])
def test_a_shard_without_a_held_out_entry(tritd, shov, monkeypatch):
    g = hc.load("hadm30_r3_tiles")
    H = g["holdout"].copy(order="F")
    H[:10] = False  # shard 0 of three: rows 0..9
    one = solve(tritd, g, holdout=H)
    monkeypatch.setenv("TRITD_SHOV", shov)
    tritd.set_devices([0, 0, 0])
    try:
        got = solve(tritd, g, holdout=H)
    finally:
        tritd.set_devices([])
    assert (got["k"], got["best_iter"], got["stop_reason"]) == (one["k"], one["best_iter"], one["stop_reason"])
    for key in ("errHist", "valHist", "valHist1"):
        np.testing.assert_allclose(got[key], one[key], rtol=hc.TOL_ERR, atol=hc.ATOL_ERR, err_msg=key)
    for key in ("A", "B", "C", "A_best", "B_best", "C_best"):
        assert rel(got[key], one[key]) <= hc.TOL_ABC, key


@pytest.mark.parametrize("case", [("cp", 6), ("cp", 11)], ids=ids([("cp", 6), ("cp", 11)]))
def test_rccl_one_rank(tritd, case):
    """One rank with a communicator: the fused schedule carries the score sums
    in the norm partials' all-reduce (r = 6), the side-stream one in red3 (r = 11)."""
    g = sweep_case(case)
    whole = solve(tritd, g)
    comm = tritd.Comm(tritd.Comm.unique_id(), 1, 0, 0)
    try:
        s = session(tritd, g, comm)
        try:
            s.run(ms.ITERS)
            got = session_result(s)
        finally:
            s.close()
    finally:
        comm.close()
    same(got, whole, ALL_KEYS)
    assert (got["k"], got["best_iter"]) == (whole["k"], whole["best_iter"])


# --- 6. refusals -----------------------------------------------------------------------------------------
def test_refusals(tritd):
    from tritd import _lib
    g = hc.load("hadm12x10x8_r2_p3")

    def refused(status, **kw):
        with pytest.raises(tritd.TritdError) as e:
            solve(tritd, g, **kw)
        assert e.value.status == status, kw.keys()
        with pytest.raises(tritd.TritdError) as e:
            session(tritd, g, **kw)
        assert e.value.status == status, kw.keys()

    D0 = g["D"].copy(order="F")
    D0[g["held_out"]] = 0.0
    cases = [dict(holdout=np.zeros(g["D"].shape, dtype=bool)),   # H & Omega empty
             dict(holdout=~g["observed"]),                       # ... flags outside Omega only
             dict(holdout=np.ones(g["D"].shape, dtype=bool)),    # Omega & ~H empty
             dict(D=D0),                                         # ||H o Omega o D|| = 0
             dict(patience=-1), dict(val_norm=0), dict(val_norm=3)]
    for kw in cases:
        refused(_lib.TRITD_ERR_ARG, **kw)
    refused(_lib.TRITD_ERR_UNSUPPORTED, opts=dict(g["opts"], model="qi"))
    with pytest.raises(tritd.TritdError) as e:  # fp32: as for any mask
        session(tritd, g, D=g["D"].astype(np.float32))
    assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED
    for shov in ("1", "0"):  # a device set: every shard refuses alike
        tritd.set_devices([0, 0])
        try:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("TRITD_SHOV", shov)
                for kw in cases:
                    with pytest.raises(tritd.TritdError) as e:
                        solve(tritd, g, **kw)
                    assert e.value.status == _lib.TRITD_ERR_ARG
        finally:
            tritd.set_devices([])
    # holdout == NULL through the C entry points themselves
    import ctypes as C
    o = tritd.api.make_opts(g["opts"])
    a = [np.asfortranarray(g[key]) for key in ("D", "A0", "B0", "C0")]
    p = [C.c_void_p(x.ctypes.data) for x in a]
    st = _lib.lib.tritd_admm_holdout_f64(p[0], None, None, 12, 10, 8, 2, C.byref(o), 0, 2, p[1], p[2], p[3],
                                         None, None, None, None, None, None, None, None, None, None, None,
                                         None, None, None, 0)
    assert st == _lib.TRITD_ERR_ARG
    h = C.c_void_p()
    st = _lib.lib.tritd_session_create_holdout(C.byref(h), 0, p[0], None, None, 12, 12, 10, 8, 0, 12, 2,
                                               C.byref(o), 0, 2, p[1], p[2], p[3], None, 0)
    assert st == _lib.TRITD_ERR_ARG and not h.value
    # the holdout getters on a session without one
    s = session(tritd, g, holdout=None)
    try:
        for f in (s.holdout_info, s.get_best, s.get_val):
            with pytest.raises(tritd.TritdError) as e:
                f()
            assert e.value.status == _lib.TRITD_ERR_STATE
        assert "valHist" not in s.get()
    finally:
        s.close()
    # the library still solves afterwards
    got = solve(tritd, g, opts=dict(g["opts"], maxIter=3, tol=0.0))
    assert got["k"] == 3 and np.isfinite(got["errHist"]).all() and np.isfinite(got["valHist1"]).all()
    np.testing.assert_allclose(got["valHist"], g["valHist"][:3], rtol=hc.TOL_ERR, atol=hc.ATOL_ERR)


# --- 7. rank selection ------------------------------------------------------------------------------------
def test_select_rank_admm_picks_the_planted_rank(tritd):
    from tritd import drivers
    c = hc.rank_selection_case()
    out = drivers.select_rank(c["X"], c["observed"], c["ranks"], c["holdout_ratio"], c["opts"], c["seed"],
                              factors=c["factors"], solver="admm", lambdas=c["lambdas"])
    res = out["results"]
    print({key: (v["min_val"], v["best_iter"], v["errHist"][-1]) for key, v in res.items()}, flush=True)
    assert out["rank"] == c["planted"] == 3 and out["lam"] in c["lambdas"]
    assert len(res) == len(c["ranks"]) * len(c["lambdas"])
    by_err = min(res, key=lambda key: res[key]["errHist"][-1])
    assert by_err[0] != c["planted"]
    best = res[(out["rank"], out["lam"])]
    assert best["min_val"] == min(v["min_val"] for v in res.values())
    H = out["holdout"]
    assert not (H & ~c["observed"]).any()
    assert H.sum() == int(np.floor(c["holdout_ratio"] * c["observed"].sum() + 0.5))
