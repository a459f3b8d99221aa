"""GPU tests of the held-out validation error and early stopping of the masked
ALS (holdout=, patience=): the fourth form of libtritd's ALS fit kernel, which
sums (X - Xhat)^2 over H & Omega in the pass that computes errHist, the holdout
finish and snapshot kernels, the sessions and the device sets, against
tests/holdout_als_oracle.py on the goldens tests/golden/hals*.npz
(tests/holdout_als_cases.py: which golden is held to what, and why)."""
import numpy as np
import pytest

import boundary_cases as bc
import holdout_als_cases as hac
import holdout_als_oracle as hao
from conftest import rel

pytestmark = pytest.mark.gpu

# one golden per padded rank (16, 32, 48, 64), the 5 t-tiles, the tiles, the ragged shape
RANK_CASES = ["hals12x10x8_r2_stop", "hals21x13x35_r5", "hals18x19x22_r6", "hals17x16x20_r8_p3"]


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


def quiet(s):
    pass


def solve(tritd, g, **kw):
    """(A, B, C, errHist, k, info) of the one-shot call on the golden's inputs."""
    args = dict(observed=g["observed"], holdout=g["holdout"], patience=g["patience"])
    args.update(kw)
    X = args.pop("X", g["X"])
    opts = args.pop("opts", g["opts"])
    return tritd.triple_decomp_ALS(X, g["r"], opts, g["A0"], g["B0"], g["C0"], return_iters=True, **args)


def masked(tritd, g, opts=None):
    return tritd.triple_decomp_ALS(g["X"], g["r"], opts or g["opts"], g["A0"], g["B0"], g["C0"],
                                   return_iters=True, observed=g["fit"])


def check_holdout(orc, got, g, name, what="", held=None):
    """Every figure printed before it is asserted."""
    A, B, C, eh, k, info = got
    held = hac.held(name) if held is None else held
    fig = dict(k=k, best_iter=info["best_iter"], stop_reason=info["stop_reason"],
               L=rel(orc.triple_product(A, B, C), orc.triple_product(g["A"], g["B"], g["C"])),
               L_best=rel(orc.triple_product(info["A_best"], info["B_best"], info["C_best"]),
                          orc.triple_product(g["A_best"], g["B_best"], g["C_best"])))
    for key, X in (("A", A), ("B", B), ("C", C), ("A_best", info["A_best"]),
                   ("B_best", info["B_best"]), ("C_best", info["C_best"])):
        fig[key] = rel(X, g[key])
    n = min(len(eh), len(g["errHist"]))
    fig["errHist"] = float(np.max(np.abs(eh[:n] - g["errHist"][:n]) / np.abs(g["errHist"][:n])))
    n = min(len(info["valHist"]), len(g["valHist"]))
    fig["valHist"] = float(np.max(np.abs(info["valHist"][:n] - g["valHist"][:n]) / np.abs(g["valHist"][:n])))
    print(name, what, " ".join("%s=%.2e" % kv for kv in fig.items()))
    assert k == g["k"] and len(eh) == g["k"] and len(info["valHist"]) == g["k"]
    assert info["best_iter"] == g["best_iter"] and info["stop_reason"] == g["stop_reason"]
    np.testing.assert_allclose(eh, g["errHist"], rtol=hac.TOL_ERR, atol=hac.ATOL_ERR)
    if "valHist" in held:
        np.testing.assert_allclose(info["valHist"], g["valHist"], rtol=hac.TOL_ERR, atol=hac.ATOL_ERR)
    assert fig["L"] <= hac.TOL_L and fig["L_best"] <= hac.TOL_L
    if "ABC" in held:
        for key in ("A", "B", "C", "A_best", "B_best", "C_best"):
            assert fig[key] <= hac.TOL_ABC, key


def same(got, ref):
    """A, B, C, errHist, k bitwise."""
    assert got[4] == ref[4]
    for a, b in zip(got[:4], ref[:4]):
        np.testing.assert_array_equal(a, b)


def same_info(a, b):
    assert (a["best_iter"], a["stop_reason"]) == (b["best_iter"], b["stop_reason"])
    for key in ("valHist", "A_best", "B_best", "C_best"):
        np.testing.assert_array_equal(a[key], b[key])


# --- 1. goldens ---------------------------------------------------------------
@pytest.mark.parametrize("name", hac.names())
def test_holdout_als_matches_golden(tritd, orc, name):
    g = hac.load(name)
    got = solve(tritd, g)
    assert got[5]["holdout_count"] == int(g["holdout_count"])
    check_holdout(orc, got, g, name)


# --- 2. the fit path is the masked one ------------------------------------------
@pytest.mark.parametrize("name", RANK_CASES + ["hals20x6x70_r3", "hals30_r3_tiles"])
def test_patience_zero_is_the_masked_call_bitwise(tritd, name):
    g = hac.load(name)
    got = solve(tritd, g, patience=0)
    same(got[:5], masked(tritd, g))
    assert got[5]["stop_reason"] == (1 if got[4] < g["opts"]["maxIter"] else 0)


# --- 3. the kernel's sum, independent of the iterates ----------------------------
def session(tritd, g, **kw):
    n1, n2, n3 = g["X"].shape
    args = dict(X=g["X"], observed=g["observed"], holdout=g["holdout"], patience=g["patience"])
    args.update(kw)
    opts = args.pop("opts", g["opts"])
    return tritd.AlsSession(g["r"], opts, g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3, **args)


@pytest.mark.parametrize("name", ["hals19x21x23_r7", "hals20x6x70_r3", "hals21x13x35_r5"])
def test_valhist_is_the_held_out_error_of_the_factors_read_before_the_step(tritd, orc, name):
    """tolerance: the rre_reference form of tests/boundary_cases.py,
    1e-12 + 2e-13 ||L|| / ||X - L|| over the held-out entries."""
    g = hac.load(name)
    H = g["held_out"]
    s = session(tritd, g, patience=0)
    try:
        cur = dict(A=g["A0"], B=g["B0"], C=g["C0"])
        for k in range(1, 5):
            L = orc.triple_product(cur["A"], cur["B"], cur["C"])
            s.run(1)
            cur = s.get()
            x, l = g["X"][H].astype(np.float64), L[H]
            ref = np.linalg.norm(x - l) / np.linalg.norm(x)
            tol = bc.RTOL_SUM + 2.0 * bc.TOL_TP * np.linalg.norm(l) / np.linalg.norm(x - l)
            got = cur["valHist"][k - 1]
            print(name, "k=%d valHist=%.17g host=%.17g rel=%.2e tol=%.2e" % (k, got, ref, abs(got - ref) / ref, tol))
            assert cur["k"] == k and len(cur["valHist"]) == k
            assert abs(got - ref) <= tol * ref
    finally:
        s.close()


# --- 4. held-out flags outside Omega ----------------------------------------------
@pytest.mark.parametrize("name", ["hals17x16x20_r8_p3", "hals30_r3_tiles"])
def test_holdout_flags_outside_observed_change_nothing(tritd, name):
    g = hac.load(name)
    ref = solve(tritd, g, holdout=g["held_out"])
    assert np.isfinite(ref[5]["valHist"]).all()
    for fill in (np.nan, np.inf):
        X = g["X"].copy(order="F")
        X[~g["observed"]] = fill
        got = solve(tritd, g, X=X, holdout=g["held_out"] | ~g["observed"])
        same(got[:5], ref[:5])
        same_info(got[5], ref[5])
        assert got[5]["holdout_count"] == ref[5]["holdout_count"]


# --- 5. counts ------------------------------------------------------------------------
def test_holdout_info_counts_real_entries_only(tritd):
    g = hac.load("hals19x21x23_r7")
    assert any(n % 16 for n in g["X"].shape)
    s = session(tritd, g)
    try:
        count, norm = s.holdout_info()
        assert count == int(g["held_out"].sum()) == int(g["holdout_count"])
        ref = np.linalg.norm(g["X"][g["held_out"]])
        assert abs(norm - ref) <= 1e-12 * ref
        assert s.mask_info() == (True, int(g["fit"].sum()))
    finally:
        s.close()


# --- 6. words all ones and all zeros ----------------------------------------------------
def test_a_whole_tile_held_out_and_an_empty_one(tritd, orc):
    g = hac.load("hals30_r3_tiles")
    obs = g["observed"].copy(order="F")
    H = g["holdout"].copy(order="F")
    obs[:16, 3, :16] = True   # tile (i 0..15, j = 3, t 0..15): every entry observed and held out
    H[:16, 3, :16] = True
    H[:16, 4, :16] = False    # tile j = 4: nothing held out
    A, B, C, eh, k, info = hao.triple_decomp_ALS_holdout(g["X"], obs, H, g["r"], g["opts"], g["A0"],
                                                         g["B0"], g["C0"], g["patience"], quiet)
    ref = dict(A=A, B=B, C=C, errHist=eh, k=k, **info)
    got = solve(tritd, g, observed=obs, holdout=H)
    assert got[5]["holdout_count"] == int((H & obs).sum())
    # (an input of this test's own: held to L, errHist and valHist like every golden)
    check_holdout(orc, got, ref, "whole tile", held=("L", "errHist", "valHist"))


# --- 7. the best iterate -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hals17x16x20_r8_p3", "hals20x6x70_r3"])
def test_best_iterate_is_the_masked_run_stopped_before_it(tritd, name):
    g = hac.load(name)
    got = solve(tritd, g)
    best = got[5]["best_iter"]
    assert best == g["best_iter"] > 1
    ref = masked(tritd, g, dict(g["opts"], maxIter=best - 1, tol=0.0))
    for key, x in zip(("A_best", "B_best", "C_best"), ref[:3]):
        np.testing.assert_array_equal(got[5][key], x)
    s = session(tritd, g)
    try:
        s.run(g["opts"]["maxIter"])
        b = s.get_best()
    finally:
        s.close()
    for key, x in zip("ABC", ref[:3]):
        np.testing.assert_array_equal(b[key], x)


def test_best_iter_one_returns_the_initial_factors(tritd):
    g = hac.load("hals12x10x8_r2_stop")
    got = solve(tritd, g, opts=dict(maxIter=1, tol=0.0))
    assert got[4] == 1 and got[5]["best_iter"] == 1 and got[5]["stop_reason"] == 0
    for key, x in (("A_best", g["A0"]), ("B_best", g["B0"]), ("C_best", g["C0"])):
        np.testing.assert_array_equal(got[5][key], x.reshape(got[5][key].shape, order="F"))
    s = session(tritd, g)
    try:
        b = s.get_best()  # before any run
        assert s.get()["best_iter"] == 0
    finally:
        s.close()
    np.testing.assert_array_equal(b["A"], g["A0"].reshape(b["A"].shape, order="F"))


# --- 8. sessions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hals17x16x20_r8_p3", "hals19x21x23_r7"])
def test_session_in_uneven_chunks_is_the_one_shot_call_bitwise(tritd, name):
    g = hac.load(name)
    whole = solve(tritd, g)
    s = session(tritd, g)
    try:
        for it in (3, 4, 1, 2, 5):
            s.run(it)
        r = s.get()
        b = s.get_best()
        if g["stop_reason"] == 2:  # run after a patience stop: a no-op
            assert s.sync() == (g["k"], True)
            s.run(3)
            r2, b2 = s.get(), s.get_best()
            assert r2["k"] == r["k"] and r2["best_iter"] == r["best_iter"]
            for key in ("A", "B", "C", "errHist", "valHist"):
                np.testing.assert_array_equal(r2[key], r[key])
            for key in "ABC":
                np.testing.assert_array_equal(b2[key], b[key])
    finally:
        s.close()
    same((r["A"], r["B"], r["C"], r["errHist"], r["k"]), whole[:5])
    same_info(dict(r, A_best=b["A"], B_best=b["B"], C_best=b["C"]), whole[5])


def test_session_with_device_masks_and_padded_leading_dimension(tritd):
    """X and both masks resident on the device, ldX = n1 + 3 (elements of X,
    bytes of the masks), the padding rows holding NaN / nonzero bytes."""
    from tritd import hip
    g = hac.load("hals19x21x23_r7")
    n1, n2, n3 = g["X"].shape
    s = session(tritd, g)
    try:
        s.run(g["opts"]["maxIter"])
        host, hbest, hinfo = s.get(), s.get_best(), s.holdout_info()
    finally:
        s.close()
    ld = n1 + 3
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
        assert s.holdout_info() == hinfo and s.mask_info() == (True, int(g["fit"].sum()))
        s.run(g["opts"]["maxIter"])
        got, best = s.get(), s.get_best()
    finally:
        s.close()
    assert (got["k"], got["best_iter"], got["stop_reason"]) == (host["k"], host["best_iter"], host["stop_reason"])
    for key in ("A", "B", "C", "errHist", "valHist"):
        np.testing.assert_array_equal(got[key], host[key])
    for key in "ABC":
        np.testing.assert_array_equal(best[key], hbest[key])


# --- 9. device sets ----------------------------------------------------------------------------------
@pytest.mark.parametrize("P,serial", [(2, False), (3, False), (2, True), (3, True)])
def test_holdout_device_set_matches_golden(tritd, orc, P, serial, monkeypatch):
    if serial:
        monkeypatch.setenv("TRITD_SHOV", "0")
    name = "hals30_r3_tiles"
    g = hac.load(name)
    assert any((g["X"].shape[0] * p // P) % 16 for p in range(1, P))
    tritd.set_devices([0] * P)
    try:
        got = solve(tritd, g)
    finally:
        tritd.set_devices([])
    check_holdout(orc, got, g, name, "P=%d%s" % (P, " serial" if serial else ""))


def test_patience_stop_on_a_device_set(tritd, orc):
    name = "hals17x16x20_r8_p3"
    g = hac.load(name)
    tritd.set_devices([0, 0])
    try:
        got = solve(tritd, g)
    finally:
        tritd.set_devices([])
    check_holdout(orc, got, g, name, "P=2")


# --- 10. refusals ----------------------------------------------------------------------------------------
def test_refusals(tritd):
    from tritd import _lib
    g = hac.load("hals12x10x8_r2_stop")

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
             dict(patience=-1)]
    for kw in cases:
        refused(_lib.TRITD_ERR_ARG, **kw)
    for serial in (False, True):  # a device set: every shard refuses alike
        tritd.set_devices([0, 0])
        try:
            with pytest.MonkeyPatch.context() as mp:
                if serial:
                    mp.setenv("TRITD_SHOV", "0")
                for kw in cases:
                    with pytest.raises(tritd.TritdError) as e:
                        solve(tritd, g, **kw)
                    assert e.value.status == _lib.TRITD_ERR_ARG
                # one shard (rows 0..5) without a held-out entry beside one with some still solves
                half = g["holdout"].copy(order="F")
                half[:6] = False
                got = solve(tritd, g, holdout=half, opts=dict(maxIter=4, tol=0.0))
                assert got[4] == 4 and np.isfinite(got[5]["valHist"]).all()
        finally:
            tritd.set_devices([])
    # the nonconvex solver has no holdout form
    with pytest.raises(tritd.TritdError) as e:
        session(tritd, g, ncvx=dict(rho=1.0, lam=0.1, gamma_A=0.01, epsilon=1e-3, p=0.5, theta=1.0))
    assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED
    # the holdout getters on a session without one
    n1, n2, n3 = g["X"].shape
    s = tritd.AlsSession(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3, X=g["X"],
                         observed=g["observed"])
    try:
        for f in (s.holdout_info, s.get_best):
            with pytest.raises(tritd.TritdError) as e:
                f()
            assert e.value.status == _lib.TRITD_ERR_STATE
        assert "valHist" not in s.get()
    finally:
        s.close()
    with pytest.raises(ValueError, match="holdout must have the shape of X"):
        solve(tritd, g, holdout=g["holdout"][:, :-1])
    # the library still solves afterwards
    got = solve(tritd, g, opts=dict(maxIter=3, tol=0.0))
    assert got[4] == 3 and np.isfinite(got[3]).all() and np.isfinite(got[5]["valHist"]).all()


# --- 11. rank selection ------------------------------------------------------------------------------------
def test_select_rank_picks_the_oracle_s_rank(tritd):
    from tritd import drivers
    c = hac.rank_selection_case()
    out = drivers.select_rank(c["X"], c["observed"], c["ranks"], c["holdout_ratio"], c["opts"], c["seed"],
                              factors=c["factors"])
    print({r: (v["min_val"], v["best_iter"]) for r, v in out["results"].items()})
    assert out["rank"] == c["planted"] == 3
    H = out["holdout"]
    assert not (H & ~c["observed"]).any() and H.sum() == round(c["holdout_ratio"] * c["observed"].sum())
