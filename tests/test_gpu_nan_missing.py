"""GPU tests of NaN as missing (observed="nan", opts.nanmissing).

The contract is bit for bit the explicit-mask call with observed = ~isnan(D),
so every comparison is np.array_equal between the "nan" call and today's call
with the byte mask on the same input Dn = where(observed, D, NaN)
(tests/nan_missing_cases.py: negative, payload and signalling NaNs included).
The shapes are the smallest that exercise what the pack kernels can get wrong:
12x10x8 (one ragged tile, padding rows and padded t), the 30^3 "tile(s)" cases
(a wholly missing tile, a ragged edge tile with no observed real row, a fully
observed tile) and 20x6x70 (several t-tiles, n2 < r^2)."""
import numpy as np
import pytest

import holdout_admm_cases as hac
import holdout_als_cases as hlc
import holdout_ncvx_cases as hnc
import masked_als_cases as mac
import masked_cases as mc
import masked_ncvx_cases as mnc
import nan_missing_cases as nm
from conftest import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def gw(tmp_path_factory):
    return nm.build_gateway(tmp_path_factory)


def same(got, ref, what=""):
    """np.array_equal on every output (tuples, with a trailing holdout dict or not)."""
    assert len(got) == len(ref)
    for q, (a, b) in enumerate(zip(got, ref)):
        if isinstance(a, dict):
            assert sorted(a) == sorted(b)
            for key in a:
                assert np.array_equal(a[key], b[key]), (what, key)
        else:
            assert np.array_equal(a, b), (what, q)


def both(call, mask):
    """(the "nan" call, today's call with the byte mask)"""
    return call("nan"), call(mask)


# --- one-shot calls ------------------------------------------------------------
def admm(tritd, g, Dn, observed, **kw):
    return tritd.triple_decomp_ADMM(Dn, g["r"], kw.pop("opts", g["opts"]), g["A0"], g["B0"], g["C0"],
                                    return_E=True, return_iters=True, observed=observed, **kw)


def als(tritd, g, Xn, observed, **kw):
    return tritd.triple_decomp_ALS(Xn, g["r"], kw.pop("opts", g["opts"]), g["A0"], g["B0"], g["C0"],
                                   return_iters=True, observed=observed, **kw)


def ncvx(tritd, g, Xn, observed, prm=None, **kw):
    return tritd.triple_decomp_ncvx(Xn, g["r"], *(prm or mnc.args(g)), g["A0"], g["B0"], g["C0"],
                                    return_iters=True, observed=observed, **kw)


@pytest.mark.parametrize("name", ["m12x10x8_r2", "m30_r3_tile", "m20x6x70_r3", "mqi12x10x8_r2"])
def test_admm_is_the_explicit_mask_call_bitwise(tritd, name):
    import tritd_oracle as orc
    g = mc.load(name)
    Dn = nm.with_nans(g["D"], g["observed"])
    got, ref = both(lambda o: admm(tritd, g, Dn, o), g["observed"])
    assert got[6] == ref[6] == g["k"]
    same(got, ref, name)
    assert not got[3][~g["observed"]].any() and not got[5][~g["observed"]].any()
    if name == "m30_r3_tile":  # and against the golden itself, not the explicit path alone
        A, B, C, O, eh, E, k = got
        fig = dict(L=rel(orc.triple_product(A, B, C), orc.triple_product(g["A"], g["B"], g["C"])),
                   O=rel(O, g["O"]), E=rel(E, g["E"]), A=rel(A, g["A"]), B=rel(B, g["B"]),
                   C=rel(C, g["C"]))
        print(name, " ".join("%s=%.2e" % kv for kv in fig.items()))
        assert max(fig["L"], fig["O"], fig["E"]) <= mc.TOL_LOE
        assert max(fig["A"], fig["B"], fig["C"]) <= mc.TOL_ABC
        np.testing.assert_allclose(eh, g["errHist"], rtol=mc.TOL_ERR, atol=mc.ATOL_ERR)


@pytest.mark.parametrize("name", ["oals12x10x8_r2", "oals30_r3_tiles", "oals20x6x70_r3"])
def test_als_is_the_explicit_mask_call_bitwise(tritd, name):
    g = mac.load(name)
    Xn = nm.with_nans(g["X"], g["observed"])
    got, ref = both(lambda o: als(tritd, g, Xn, o), g["observed"])
    assert got[4] == g["k"]
    same(got, ref, name)


@pytest.mark.parametrize("name", ["onc12x10x8_r2", "onc30_r3_tiles"])
def test_ncvx_is_the_explicit_mask_call_bitwise(tritd, name):
    g = mnc.load(name)
    Xn = nm.with_nans(g["X"], g["observed"])
    got, ref = both(lambda o: ncvx(tritd, g, Xn, o), g["observed"])
    assert got[5] == g["k"]
    same(got, ref, name)
    assert not got[3][~g["observed"]].any()


# --- holdout: both histories, best_iter, stop_reason, the best factors, the count --
def holdout_inputs(g, key):
    """Dn, and H with a few more flags at NaN entries (ignored: only H & Omega counts)."""
    H = nm.holdout_with_flags_outside(g["holdout"], g["observed"])
    return nm.with_nans(g[key], g["observed"]), H


@pytest.mark.parametrize("name", ["hadm12x10x8_r2_p3", "hadm30_r3_tiles"])
def test_admm_holdout_is_the_explicit_mask_call_bitwise(tritd, name):
    g = hac.load(name)
    Dn, H = holdout_inputs(g, "D")
    kw = dict(holdout=H, patience=g["patience"], val_norm=g["val_norm"])
    got, ref = both(lambda o: admm(tritd, g, Dn, o, **kw), g["observed"])
    same(got, ref, name)
    v = got[-1]
    assert v["holdout_count"] == int(g["held_out"].sum())
    assert (got[6], v["best_iter"], v["stop_reason"]) == (g["k"], g["best_iter"], g["stop_reason"])


@pytest.mark.parametrize("name", ["hals12x10x8_r2_stop", "hals30_r3_tiles"])
def test_als_holdout_is_the_explicit_mask_call_bitwise(tritd, name):
    g = hlc.load(name)
    Xn, H = holdout_inputs(g, "X")
    kw = dict(holdout=H, patience=g["patience"])
    got, ref = both(lambda o: als(tritd, g, Xn, o, **kw), g["observed"])
    same(got, ref, name)
    v = got[-1]
    assert v["holdout_count"] == int(g["held_out"].sum())
    assert (got[4], v["best_iter"], v["stop_reason"]) == (g["k"], g["best_iter"], g["stop_reason"])


@pytest.mark.parametrize("name", ["hnc12x10x8_r2_p", "hnc30_r3_tiles"])
def test_ncvx_holdout_is_the_explicit_mask_call_bitwise(tritd, name):
    g = hnc.load(name)
    Xn, H = holdout_inputs(g, "X")
    kw = dict(holdout=H, patience=g["patience"], val_norm=g["val_norm"], prm=hnc.args(g))
    got, ref = both(lambda o: ncvx(tritd, g, Xn, o, **kw), g["observed"])
    same(got, ref, name)
    v = got[-1]
    assert v["holdout_count"] == int(g["held_out"].sum())
    assert (got[5], v["best_iter"], v["stop_reason"]) == (g["k"], g["best_iter"], g["stop_reason"])


# --- sessions --------------------------------------------------------------------
SESSION_CASES = {"admm": (mc, "m30_r3_tile", "D"), "als": (mac, "oals30_r3_tiles", "X"),
                 "als_ncvx": (mnc, "onc12x10x8_r2", "X"), "ncvx_holdout": (hnc, "hnc12x10x8_r2_p", "X")}


def session_case(kind):
    """The golden of a session kind, with Dn and (the NcvxSession) its holdout."""
    mod, name, key = SESSION_CASES[kind]
    g = mod.load(name)
    g["Dn"] = nm.with_nans(g[key], g["observed"])
    g["H"] = nm.holdout_with_flags_outside(g["holdout"], g["observed"]) if "holdout" in g else None
    return g


def make_session(tritd, kind, g, observed, dev=None):
    """dev: a dict that receives the device buffers of a device-resident tensor
    at ld = n1 + 5, its padding rows NaN (and nonzero holdout bytes)."""
    from tritd import hip
    Dn, H = g["Dn"], g["H"]
    n1, n2, n3 = Dn.shape
    kw = dict(n1=n1, n2=n2, n3=n3, device=0, observed=observed)
    if dev is not None:
        ld = n1 + 5
        Dp = np.full((ld, n2, n3), np.nan, order="F")
        Dp.view(np.uint64)[:n1] = Dn.view(np.uint64)  # (the bits: no NaN is quieted)
        dev["D"] = hip.DeviceArray.from_host(Dp)
        kw.update({"d_device_ptr" if kind == "admm" else "x_device_ptr": dev["D"].ptr,
                   "ldD" if kind == "admm" else "ldX": ld})
        if H is not None:
            Hp = np.full((ld, n2, n3), 0xFF, dtype=np.uint8, order="F")
            Hp[:n1] = H
            dev["H"] = hip.DeviceArray.from_host(Hp)
            H = dev["H"].ptr
    else:
        kw["D" if kind == "admm" else "X"] = Dn
    f = (g["A0"], g["B0"], g["C0"])
    o = dict(g["opts"], maxIter=10)
    if kind == "admm":
        return tritd.Session(g["r"], o, *f, probe=False, **kw)
    if kind == "als":
        return tritd.AlsSession(g["r"], o, *f, **kw)
    if kind == "als_ncvx":
        return tritd.AlsSession(g["r"], o, *f, ncvx=mnc.ncvx_dict(mnc.args(g)), **kw)
    return tritd.NcvxSession(g["r"], o, *f, ncvx=hnc.ncvx_dict(hnc.args(g)), holdout=H,
                             patience=g["patience"], val_norm=g["val_norm"], **kw)


def stepped(s, kind):
    """3 + 7 iterations, then everything the session returns."""
    try:
        s.run(3)
        s.sync()
        s.run(7)
        out = dict(s.get())
        out["mask_info"] = s.mask_info()
        if kind in ("als_ncvx", "ncvx_holdout"):
            out["O"] = s.get_O()
        if kind == "ncvx_holdout":
            out["best"] = s.get_best()
            out["holdout_info"] = s.holdout_info()
        return out
    finally:
        s.close()


def same_dict(a, b, what):
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], dict):
            same_dict(a[key], b[key], what + "." + key)
        else:
            assert np.array_equal(a[key], b[key]), (what, key)


@pytest.fixture(scope="module")
def explicit_sessions(tritd):
    """kind -> (its case, the explicit-mask session stepped 3 + 7), computed once per kind."""
    cache = {}

    def get(kind):
        if kind not in cache:
            g = session_case(kind)
            cache[kind] = (g, stepped(make_session(tritd, kind, g, g["observed"]), kind))
        return cache[kind]

    return get


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("kind", sorted(SESSION_CASES))
def test_sessions_stepped_match_the_explicit_mask_sessions(tritd, explicit_sessions, kind, where):
    g, ref = explicit_sessions(kind)
    dev = {} if where == "device" else None
    try:
        s = make_session(tritd, kind, g, "nan", dev)
    finally:  # (the session has its own tile-major copy)
        for b in (dev or {}).values():
            b.free()
    got = stepped(s, kind)
    # the derived |Omega|; a holdout session reports its two parts, |Omega & ~H|
    # in mask_info and |H & Omega| in holdout_info (include/tritd.h)
    held = got["holdout_info"][0] if "holdout_info" in got else 0
    assert got["mask_info"][0] is True
    assert got["mask_info"][1] + held == int(np.count_nonzero(~np.isnan(g["Dn"])))
    assert held == (int((g["H"] & g["observed"]).sum()) if g["H"] is not None else 0)
    assert got["k"] >= 4  # the second run() continued the first
    same_dict(got, ref, kind + " " + where)


# --- the device set: mode-1 shards, one device repeated -------------------------
def first_shard_missing(g, key):
    """The mask with rows 0..9 (the first of three shards of n1 = 30) unobserved."""
    obs = g["observed"].copy()
    obs[:10] = False
    return nm.with_nans(g[key], obs), obs


@pytest.mark.parametrize("variant", ["golden", "first_shard_all_nan"])
@pytest.mark.parametrize("solver,shov", [("admm", None), ("admm", "0"), ("als", None), ("ncvx", None)])
def test_device_set_passes_the_constant_through(tritd, solver, shov, variant, monkeypatch):
    if shov is not None:
        monkeypatch.setenv("TRITD_SHOV", shov)
    g, key, call = {"admm": (mc.load("m30_r3_tile"), "D", admm),
                    "als": (mac.load("oals30_r3_tiles"), "X", als),
                    "ncvx": (mnc.load("onc30_r3_tiles"), "X", ncvx)}[solver]
    if variant == "golden":
        Dn, obs = nm.with_nans(g[key], g["observed"]), g["observed"]
    else:
        Dn, obs = first_shard_missing(g, key)
    tritd.set_devices([0, 0, 0])
    try:
        got, ref = both(lambda o: call(tritd, g, Dn, o), obs)
    finally:
        tritd.set_devices([])
    same(got, ref, "%s %s shov=%s" % (solver, variant, shov))
    assert np.isfinite(got[3 if solver == "als" else 4]).all()  # errHist


def test_device_set_holdout_passes_the_constant_through(tritd):
    g = hac.load("hadm30_r3_tiles")
    Dn, H = holdout_inputs(g, "D")
    kw = dict(holdout=H, patience=g["patience"], val_norm=g["val_norm"])
    tritd.set_devices([0, 0, 0])
    try:
        got, ref = both(lambda o: admm(tritd, g, Dn, o, **kw), g["observed"])
    finally:
        tritd.set_devices([])
    same(got, ref, "hadm30_r3_tiles P=3")


# --- Inf is data; an all-NaN tensor has nothing to fit ---------------------------
def test_inf_counts_as_observed(tritd):
    g = mc.load("m12x10x8_r2")
    Dn = nm.with_nans(g["D"], g["observed"])
    idx = np.argwhere(g["observed"])
    Dn[tuple(idx[0])], Dn[tuple(idx[-1])] = np.inf, -np.inf
    count = int(np.count_nonzero(~np.isnan(Dn)))
    assert count == int(g["observed"].sum())
    kw = dict(n1=12, n2=10, n3=8, device=0, observed="nan")
    s = tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], D=Dn, probe=False, **kw)
    try:
        assert s.mask_info() == (True, count)
    finally:
        s.close()
    s = tritd.AlsSession(g["r"], dict(maxIter=3, tol=0.0), g["A0"], g["B0"], g["C0"], X=Dn, **kw)
    try:
        assert s.mask_info() == (True, count)
    finally:
        s.close()


def test_all_nan_is_an_argument_error(tritd):
    from tritd import _lib
    g = mc.load("m30_r3_tile")
    Dn = nm.with_nans(g["D"], np.zeros(g["D"].shape, dtype=bool))
    f = (g["A0"], g["B0"], g["C0"])
    kw = dict(n1=30, n2=30, n3=30, device=0, observed="nan")
    calls = [lambda: admm(tritd, g, Dn, "nan"),
             lambda: tritd.triple_decomp_ALS(Dn, g["r"], dict(maxIter=3, tol=0.0), *f, observed="nan"),
             lambda: tritd.Session(g["r"], g["opts"], *f, D=Dn, probe=False, **kw),
             lambda: tritd.AlsSession(g["r"], dict(maxIter=3, tol=0.0), *f, X=Dn, **kw)]
    for call in calls:
        with pytest.raises(tritd.TritdError) as e:
            call()
        assert e.value.status == _lib.TRITD_ERR_ARG
    tritd.set_devices([0, 0, 0])
    try:
        for call in calls[:2]:
            with pytest.raises(tritd.TritdError) as e:
                call()
            assert e.value.status == _lib.TRITD_ERR_ARG
    finally:
        tritd.set_devices([])
    # the library still solves afterwards
    got = admm(tritd, g, nm.with_nans(g["D"], g["observed"]), "nan", opts=dict(g["opts"], maxIter=3))
    assert got[6] == 3 and np.isfinite(got[4]).all()


# --- the MEX gateway: opts.nanmissing is what turns the mask on -------------------
def test_gateway_admm_with_nanmissing_matches_the_golden(tritd, gw):
    import tritd_oracle as orc
    g = mc.load("m30_r3_tile")
    Dn = nm.with_nans(g["D"], g["observed"])
    vals = [float(g["opts"][n]) for n in nm.ADMM_FIELDS]
    rc, err, res = nm.gateway_admm(gw, g, Dn, nm.ADMM_FIELDS + ["nanmissing"], vals + [1.0])
    assert rc == 0, err
    assert res["k"] == g["k"]
    fig = dict(L=rel(orc.triple_product(res["A"], res["B"], res["C"]),
                     orc.triple_product(g["A"], g["B"], g["C"])),
               O=rel(res["O"], g["O"]), E=rel(res["E"], g["E"]))
    print(" ".join("%s=%.2e" % kv for kv in fig.items()))
    assert fig["L"] <= 1e-9 and fig["O"] <= 1e-9 and fig["E"] <= 1e-9
    np.testing.assert_allclose(res["errHist"], g["errHist"], rtol=1e-8, atol=1e-13)
    # and it is the Python call, bit for bit
    ref = admm(tritd, g, Dn, "nan")
    for key, q in (("A", 0), ("B", 1), ("C", 2), ("O", 3), ("errHist", 4), ("E", 5)):
        assert np.array_equal(res[key], ref[q]), key
    # without the field the NaNs are data
    rc, err, res = nm.gateway_admm(gw, g, Dn, nm.ADMM_FIELDS, vals)
    assert rc == 0, err
    assert np.isnan(res["A"]).any() and np.isnan(res["O"]).any() and np.isnan(res["errHist"]).all()
    # a single D with the field: the library's refusal
    rc, err, _ = nm.gateway_admm(gw, g, Dn, nm.ADMM_FIELDS + ["nanmissing"], vals + [1.0], single=True)
    assert rc == 1 and err.startswith("tritd:solver|") and "double D only" in err
    # nanmissing = 0 is the field left out, for a double and for a single D
    for single in (False, True):
        rc0, err0, r0 = nm.gateway_admm(gw, g, g["D"], nm.ADMM_FIELDS + ["nanmissing"], vals + [0.0],
                                        single=single)
        rc1, err1, r1 = nm.gateway_admm(gw, g, g["D"], nm.ADMM_FIELDS, vals, single=single)
        assert rc0 == rc1 == 0, (err0, err1)
        for key in r0:
            assert np.array_equal(r0[key], r1[key]), (single, key)


def test_gateway_als_with_nanmissing_matches_the_golden(tritd, gw):
    import tritd_oracle as orc
    g = mac.load("oals30_r3_tiles")
    Xn = nm.with_nans(g["X"], g["observed"])
    vals = [float(g["opts"]["maxIter"]), float(g["opts"]["tol"])]
    rc, err, res = nm.gateway_als(gw, g, Xn, ["maxIter", "tol", "nanmissing"], vals + [1.0])
    assert rc == 0, err
    assert res["k"] == g["k"]
    d = rel(orc.triple_product(res["A"], res["B"], res["C"]), orc.triple_product(g["A"], g["B"], g["C"]))
    print("L=%.2e" % d)
    assert d <= 1e-9
    np.testing.assert_allclose(res["errHist"], g["errHist"], rtol=1e-8, atol=1e-13)
    rc, err, res = nm.gateway_als(gw, g, Xn, ["maxIter", "tol"], vals)
    assert rc == 0, err
    assert np.isnan(res["A"]).any() and np.isnan(res["errHist"]).all()
