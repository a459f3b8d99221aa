"""Held-out validation of the masked nonconvex solver on the GPU (holdout=,
patience=, val_norm=; include/tritd.h: tritd_ncvx_holdout_f64).

Reference: tests/holdout_ncvx_oracle.py through the goldens of
tests/holdout_ncvx_cases.py, at the tolerances tests/masked_ncvx_cases.py uses
for the onc* goldens (L, O, A, B, C <= 1e-9; errHist, valHist, valHist1 within
1e-8 |ref| + 1e-13; the same k, best_iter and stop_reason), and the masked call
itself (triple_decomp_ncvx(observed = Omega & ~H)), bit for bit.
"""
import numpy as np
import pytest

import boundary_cases as bc
import holdout_ncvx_cases as hc

pytestmark = pytest.mark.gpu

FIT_KEYS = ("A", "B", "C", "O", "errHist")
ALL_KEYS = FIT_KEYS + ("valHist", "valHist1", "A_best", "B_best", "C_best")
# one golden per padded rank (RP = 16, 32, 48, 64)
PER_RP = ["hnc20x6x70_r3_l1", "hnc21x13x35_r5", "hnc18x19x22_r6", "hnc17x16x20_r8_stop"]
SMALL = "hnc12x10x8_r2_p"


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


def gate(a, b):
    return float(np.max(np.abs(a - b) / (hc.RTOL_ERR * np.abs(b) + hc.ATOL_ERR)))


def solve(tritd, g, **kw):
    """dict(A, B, C, O, errHist, k, + the holdout dict) of the one-shot call."""
    a = dict(observed=g["observed"], holdout=g["holdout"], patience=g["patience"], val_norm=g["val_norm"],
             X=g["X"], over={})
    a.update(kw)
    X, over = a.pop("X"), a.pop("over")
    A, B, C, O, eh, k, v = tritd.triple_decomp_ncvx(X, g["r"], *hc.args(g, **over), g["A0"], g["B0"], g["C0"],
                                                    return_iters=True, **a)
    return dict(v, A=A, B=B, C=C, O=O, errHist=eh, k=k)


def solve_masked(tritd, g, **over):
    A, B, C, O, eh, k = tritd.triple_decomp_ncvx(g["X"], g["r"], *hc.args(g, **over), g["A0"], g["B0"], g["C0"],
                                                 return_iters=True, observed=g["fit"])
    return dict(A=A, B=B, C=C, O=O, errHist=eh, k=k)


def session(tritd, g, comm=None, **kw):
    n1, n2, n3 = g["X"].shape
    a = dict(X=g["X"], observed=g["observed"], holdout=g["holdout"], patience=g["patience"],
             val_norm=g["val_norm"], over={})
    a.update(kw)
    prm = hc.args(g, **a.pop("over"))
    return tritd.NcvxSession(g["r"], dict(maxIter=prm[6], tol=prm[7]), g["A0"], g["B0"], g["C0"], n1=n1, n2=n2,
                             n3=n3, device=0, comm=comm, ncvx=hc.ncvx_dict(prm), **a)


def session_result(s):
    x = s.get()
    b = s.get_best()
    return dict(x, O=s.get_O(), A_best=b["A"], B_best=b["B"], C_best=b["C"])


def same(got, ref, keys):
    for key in keys:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


def check(orc, got, g, what=""):
    """Every figure printed before it is asserted."""
    fig = dict(k=got["k"], best=got["best_iter"], stop=got["stop_reason"],
               L=hc.rel(orc.triple_product(got["A"], got["B"], got["C"]),
                        orc.triple_product(g["A"], g["B"], g["C"])),
               O=hc.rel(got["O"], g["O"]))
    for key in ("A", "B", "C", "A_best", "B_best", "C_best"):
        fig[key] = hc.rel(got[key], g[key])
    n = {key: min(len(got[key]), len(g[key])) for key in ("errHist", "valHist", "valHist1")}
    for key in n:
        fig[key] = gate(got[key][:n[key]], g[key][:n[key]])
    print(g["name"], what, " ".join("%s=%.2e" % kv for kv in fig.items()), flush=True)
    assert (got["k"], got["best_iter"], got["stop_reason"]) == (g["k"], g["best_iter"], g["stop_reason"])
    for key in n:
        assert len(got[key]) == g["k"]
        np.testing.assert_allclose(got[key], g[key], rtol=hc.RTOL_ERR, atol=hc.ATOL_ERR, err_msg=key)
    for key in ("L", "O", "A", "B", "C", "A_best", "B_best", "C_best"):
        assert fig[key] <= hc.TOL, key
    assert not got["O"][~g["fit"]].any()  # held out or unobserved
    if "holdout_count" in got:
        assert got["holdout_count"] == int(g["held_out"].sum())


# --- 1. the goldens ---------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.names())
def test_holdout_ncvx_matches_golden(tritd, orc, name):
    g = hc.load(name)
    check(orc, solve(tritd, g), g, "one-shot")


# --- 2. patience = 0 is the masked call, bit for bit ----------------------------------------
@pytest.mark.parametrize("name", PER_RP + ["hnc30_r3_tiles"])
def test_patience_zero_is_the_masked_call_bitwise(tritd, name):
    g = hc.load(name)
    assert name == "hnc30_r3_tiles" or hc.padded_rank(g["r"]) == 16 * (1 + PER_RP.index(name))
    got = solve(tritd, g, patience=0)
    ref = solve_masked(tritd, g)
    assert got["k"] == ref["k"] == g["k"]
    same(got, ref, FIT_KEYS)
    out = ~g["fit"]
    assert not got["O"][out].any() and np.any(got["O"]) and g["held_out"].any()


# --- 3. the scores step by step (the XT slot map), the best iterate --------------------------------
def host_scores(orc, g, f):
    """((valHist, rtol), (valHist1, rtol)) of the factors f on the host.  The l2
    sums and their tolerances are boundary_cases.rre_reference's, halved by the
    square root; the l1 numerator moves by at most TOL_TP sum |T| when the MFMA
    product T moves by TOL_TP |T| elementwise, and each sum by RTOL_SUM."""
    x = g["X"][g["held_out"]]
    t = orc.triple_product(*f)[g["held_out"]]
    num, den, rnum, rden = bc.rre_reference(t, x)
    a1 = float(np.abs(x - t).sum())
    r1 = 2.0 * bc.RTOL_SUM + bc.TOL_TP * float(np.abs(t).sum()) / a1
    return (np.sqrt(num / den), 0.5 * (rnum + rden)), (a1 / float(np.abs(x).sum()), r1)


@pytest.mark.parametrize("name", PER_RP + ["hnc30_r3_tiles"])
def test_scores_against_the_host_from_the_factors_read_before_each_step(tritd, orc, name):
    g = hc.load(name)
    x = g["X"][g["held_out"]]
    s = session(tritd, g, patience=0, over=dict(tol=0.0))
    try:
        cnt, nrm = s.holdout_info()
        assert cnt == int(g["held_out"].sum()) and abs(nrm - np.linalg.norm(x)) <= 1e-13 * nrm
        assert s.mask_info() == (True, int(g["fit"].sum()))
        assert s.get_val()["best_iter"] == 0
        same(s.get_best(), dict(A=g["A0"], B=g["B0"], C=g["C0"]), "ABC")
        worst = 0.0
        steps = min(6, g["opts"]["maxIter"])
        for k in range(1, steps + 1):
            before = s.get()
            s.run(1)
            v = s.get_val()
            assert len(v["valHist"]) == len(v["valHist1"]) == k
            (v2, r2), (v1, r1) = host_scores(orc, g, (before["A"], before["B"], before["C"]))
            fig = (abs(v["valHist"][-1] - v2) / (r2 * v2), abs(v["valHist1"][-1] - v1) / (r1 * v1))
            print("  %s step %d valHist %.3e (host %.3e, %.2f of rtol %.1e) valHist1 %.3e (host %.3e, %.2f of "
                  "rtol %.1e)" % (name, k, v["valHist"][-1], v2, fig[0], r2, v["valHist1"][-1], v1, fig[1], r1),
                  flush=True)
            worst = max(worst, *fig)
        assert worst <= 1.0
    finally:
        s.close()


@pytest.mark.parametrize("name", [SMALL, "hnc17x16x20_r8_stop", "hnc21x13x35_r5"])
def test_get_best_is_the_masked_run_of_best_iter_minus_one_bitwise(tritd, name):
    g = hc.load(name)
    got = solve(tritd, g)
    assert got["best_iter"] == g["best_iter"] > 1
    ref = solve_masked(tritd, g, maxIter=g["best_iter"] - 1, tol=0.0)
    assert ref["k"] == g["best_iter"] - 1
    for key in "ABC":
        np.testing.assert_array_equal(got[key + "_best"], ref[key])
    # a stop of either kind leaves the updates of k and O of k-1
    cut = solve_masked(tritd, g, maxIter=g["k"], tol=0.0)
    same(got, cut, ("A", "B", "C"))
    np.testing.assert_array_equal(got["errHist"], cut["errHist"][:g["k"]])
    if g["stop_reason"]:
        np.testing.assert_array_equal(got["O"], solve_masked(tritd, g, maxIter=g["k"] - 1, tol=0.0)["O"])
    else:
        np.testing.assert_array_equal(got["O"], cut["O"])


def test_best_iter_one_keeps_the_initial_factors(tritd):
    g = hc.load(SMALL)
    got = solve(tritd, g, patience=0, over=dict(maxIter=1))
    assert (got["k"], got["best_iter"], got["stop_reason"]) == (1, 1, 0)
    same(dict(A=got["A_best"], B=got["B_best"], C=got["C_best"]), dict(A=g["A0"], B=g["B0"], C=g["C0"]), "ABC")


def test_val_norm_picks_the_history(tritd):
    g = hc.load(SMALL)
    # (the golden's own five iterations: their decision margins are admitted)
    a = solve(tritd, g, patience=0, val_norm=2, over=dict(maxIter=g["k"]))
    b = solve(tritd, g, patience=0, val_norm=1, over=dict(maxIter=g["k"]))
    assert (g["best_iter"], g["best_iter_other"]) == (a["best_iter"], b["best_iter"])
    same(a, b, FIT_KEYS + ("valHist", "valHist1"))
    assert a["best_iter"] == 1 + int(np.argmin(a["valHist"])) != b["best_iter"] == 1 + int(np.argmin(a["valHist1"]))


# --- 4. fill values, sessions -----------------------------------------------------------------------
def test_nan_and_inf_at_flags_outside_omega(tritd):
    g = hc.load("hnc30_r3_tiles")
    ref = solve(tritd, g)
    miss = ~g["observed"]
    assert (g["holdout"] & miss).any()
    for fill in (np.nan, np.inf):
        X = g["X"].copy(order="F")
        X[miss] = fill
        got = solve(tritd, g, X=X, holdout=g["holdout"] | miss)
        same(got, ref, ALL_KEYS)
        assert (got["k"], got["best_iter"], got["holdout_count"]) == (ref["k"], ref["best_iter"],
                                                                      int(g["held_out"].sum()))


def test_session_stepped_3_plus_7_against_10(tritd):
    g = hc.load("hnc18x19x22_r6")
    whole = solve(tritd, g)
    s = session(tritd, g)
    try:
        s.run(3)
        s.run(7)
        got = session_result(s)
        ms = s.holdout_ms()
    finally:
        s.close()
    same(got, whole, ALL_KEYS)
    assert (got["k"], got["best_iter"], got["stop_reason"]) == (10, whole["best_iter"], 0)
    assert ms == dict(score=0.0, tail=0.0)  # (timing is off)


def test_a_run_after_a_patience_stop_is_a_no_op(tritd, orc):
    g = hc.load(SMALL)
    s = session(tritd, g)
    try:
        s.run(g["opts"]["maxIter"])
        got = session_result(s)
        assert s.sync() == (g["k"], True)
        s.run(3)
        again = session_result(s)
    finally:
        s.close()
    check(orc, got, g, "session")
    same(again, got, ALL_KEYS)
    assert (again["k"], again["best_iter"], again["stop_reason"]) == (got["k"], got["best_iter"], 2)


def test_a_run_after_a_stop_of_line_65_is_a_no_op(tritd, orc):
    g = hc.load("hnc17x16x20_r8_stop")
    s = session(tritd, g)
    try:
        s.set_timing(True)
        s.run(g["opts"]["maxIter"])
        got = session_result(s)
        ms = s.holdout_ms()
        s.run(2)
        again = session_result(s)
    finally:
        s.close()
    check(orc, got, g, "session, timed")
    same(again, got, ALL_KEYS)
    assert (again["k"], again["best_iter"], again["stop_reason"]) == (got["k"], got["best_iter"], 1)
    assert 0.0 < ms["score"] <= ms["tail"]


def test_session_with_device_masks_and_padded_leading_dimension(tritd):
    """X and both masks resident on the device, ldX = n1 + 5 (elements of X,
    bytes of the masks), the padding rows holding NaN / nonzero bytes."""
    from tritd import hip
    g = hc.load("hnc21x13x35_r5")
    whole = solve(tritd, g)
    n1, n2, n3 = g["X"].shape
    ld = n1 + 5
    Xp = np.full((ld, n2, n3), np.nan, order="F")
    Xp[:n1] = g["X"]
    Mp = np.full((ld, n2, n3), 0xFF, dtype=np.uint8, order="F")
    Mp[:n1] = g["observed"]
    Hp = np.full((ld, n2, n3), 0xFF, dtype=np.uint8, order="F")
    Hp[:n1] = g["holdout"]
    dev = [hip.DeviceArray.from_host(x) for x in (Xp, Mp, Hp)]
    try:
        s = session(tritd, g, X=None, x_device_ptr=dev[0].ptr, ldX=ld, observed=dev[1].ptr, holdout=dev[2].ptr)
    finally:
        for d in dev:
            d.free()
    try:
        assert s.holdout_info()[0] == int(g["held_out"].sum())
        assert s.mask_info() == (True, int(g["fit"].sum()))
        s.run(g["opts"]["maxIter"])
        got = session_result(s)
    finally:
        s.close()
    same(got, whole, ALL_KEYS)
    assert got["best_iter"] == whole["best_iter"]


# --- 5. shards ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shov", ["1", "0"])
@pytest.mark.parametrize("name", ["hnc30_r3_tiles", SMALL, "hnc17x16x20_r8_stop"])
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
    g = hc.load("hnc30_r3_tiles")
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
        np.testing.assert_allclose(got[key], one[key], rtol=hc.RTOL_ERR, atol=hc.ATOL_ERR, err_msg=key)
    for key in ("A", "B", "C", "O", "A_best", "B_best", "C_best"):
        assert hc.rel(got[key], one[key]) <= hc.TOL, key


@pytest.mark.parametrize("name", ["hnc18x19x22_r6", SMALL])
def test_rccl_one_rank(tritd, name):
    """One rank with a communicator: the score sums ride in the fit sums' all-reduce."""
    g = hc.load(name)
    whole = solve(tritd, g)
    comm = tritd.Comm(tritd.Comm.unique_id(), 1, 0, 0)
    try:
        s = session(tritd, g, comm)
        try:
            s.run(g["opts"]["maxIter"])
            got = session_result(s)
        finally:
            s.close()
    finally:
        comm.close()
    same(got, whole, ALL_KEYS)
    assert (got["k"], got["best_iter"], got["stop_reason"]) == (whole["k"], whole["best_iter"], whole["stop_reason"])


# --- 6. refusals -----------------------------------------------------------------------------------------
def test_refusals(tritd):
    import ctypes as C

    from tritd import _lib
    g = hc.load(SMALL)

    def refused(status, **kw):
        with pytest.raises(tritd.TritdError) as e:
            solve(tritd, g, **kw)
        assert e.value.status == status, kw.keys()
        with pytest.raises(tritd.TritdError) as e:
            session(tritd, g, **kw)
        assert e.value.status == status, kw.keys()

    X0 = g["X"].copy(order="F")
    X0[g["held_out"]] = 0.0
    cases = [dict(holdout=np.zeros(g["X"].shape, dtype=bool)),   # H & Omega empty
             dict(holdout=~g["observed"]),                       # ... flags outside Omega only
             dict(holdout=np.ones(g["X"].shape, dtype=bool)),    # Omega & ~H empty
             dict(X=X0),                                         # ||H o Omega o X|| = 0
             dict(patience=-1), dict(val_norm=0), dict(val_norm=3), dict(over=dict(rho=0.0))]
    for kw in cases:
        refused(_lib.TRITD_ERR_ARG, **kw)
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
    # r > 8
    n1, n2, n3 = g["X"].shape
    rng = np.random.default_rng(9)
    f9 = [np.asfortranarray(rng.standard_normal(s)) for s in ((n1, 9, 9), (9, n2, 9), (9, 9, n3))]
    with pytest.raises(tritd.TritdError) as e:
        tritd.triple_decomp_ncvx(g["X"], 9, *hc.args(g), *f9, observed=g["observed"], holdout=g["holdout"])
    assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED
    # holdout == NULL through the C entry points themselves
    o = tritd.api.make_als_opts(dict(maxIter=5, tol=0.0))
    a = [np.asfortranarray(g[key]) for key in ("X", "A0", "B0", "C0")]
    p = [C.c_void_p(x.ctypes.data) for x in a]
    out = [np.zeros_like(x) for x in (a[1], a[2], a[3], a[0])] + [np.zeros(5)]
    po = [C.c_void_p(x.ctypes.data) for x in out]
    st = _lib.lib.tritd_ncvx_holdout_f64(p[0], None, None, 12, 10, 8, 2, 1.0, 0.5, 1e-3, 1e-2, 0.5, 2.0 / 3.0, 5,
                                         0.0, 0, 2, p[1], p[2], p[3], *po, None, None, None, None, None, None,
                                         None, None, 0)
    assert st == _lib.TRITD_ERR_ARG
    h = C.c_void_p()
    st = _lib.lib.tritd_als_session_create_ncvx_holdout(C.byref(h), 0, p[0], None, None, 12, 12, 10, 8, 0, 12, 2,
                                                        C.byref(o), 0, 2, 1.0, 0.5, 1e-3, 1e-2, 0.5, 2.0 / 3.0,
                                                        p[1], p[2], p[3], None, 0, 1)
    assert st == _lib.TRITD_ERR_ARG and not h.value
    # the ALS holdout session still refuses the nonconvex solver, both ways
    with pytest.raises(tritd.TritdError) as e:
        tritd.AlsSession(g["r"], dict(maxIter=5, tol=0.0), g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3,
                         X=g["X"], observed=g["observed"], holdout=g["holdout"], ncvx=hc.ncvx_dict(hc.args(g)))
    assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED
    s = tritd.AlsSession(g["r"], dict(maxIter=5, tol=0.0), g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3,
                         X=g["X"], observed=g["observed"], holdout=g["holdout"])
    try:
        with pytest.raises(tritd.TritdError) as e:
            s.set_ncvx(*hc.args(g)[:6])
        assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED
        # and the new getters are for the new session only
        for f in (lambda: _lib.lib.tritd_als_session_get_val2(s._s, None, None, None, None),
                  lambda: _lib.lib.tritd_als_session_holdout_ms(s._s, None, None)):
            assert f() == _lib.TRITD_ERR_STATE
    finally:
        s.close()
    # the solver of a nonconvex holdout session is fixed at creation
    s = session(tritd, g)
    try:
        with pytest.raises(tritd.TritdError) as e:
            s.set_ncvx(*hc.args(g)[:6])
        assert e.value.status == _lib.TRITD_ERR_STATE
    finally:
        s.close()
    # the library still solves afterwards
    got = solve(tritd, g, patience=0, over=dict(maxIter=3))
    assert got["k"] == 3 and np.isfinite(got["errHist"]).all() and np.isfinite(got["valHist1"]).all()
    np.testing.assert_allclose(got["valHist"], g["valHist"][:3], rtol=hc.RTOL_ERR, atol=hc.ATOL_ERR)


# --- 7. rank selection ------------------------------------------------------------------------------------
def test_select_rank_ncvx_picks_the_planted_rank(tritd):
    from tritd import drivers
    c = hc.rank_selection_case()
    out = drivers.select_rank(c["X"], c["observed"], c["ranks"], c["holdout_ratio"], c["opts"], c["seed"],
                              factors=c["factors"], solver="ncvx", gammas=c["gammas"])
    res = out["results"]
    print({key: (v["min_val"], v["best_iter"], v["errHist"][-1]) for key, v in res.items()}, flush=True)
    assert out["rank"] == c["planted"] == 3 and out["gamma_A"] == c["gammas"][0] and out["lam"] == c["opts"]["lam"]
    assert len(res) == len(c["ranks"]) * len(c["gammas"])
    by_err = min(res, key=lambda key: res[key]["errHist"][-1])
    assert by_err[0] != c["planted"]
    best = res[(out["rank"], out["lam"], out["gamma_A"])]
    assert best["min_val"] == min(v["min_val"] for v in res.values())
    H = out["holdout"]
    assert not (H & ~c["observed"]).any()
    assert H.sum() == int(np.floor(c["holdout_ratio"] * c["observed"].sum() + 0.5))
