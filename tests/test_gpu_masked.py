"""GPU tests of the mask-aware ADMM (opts.observed): libtritd's masked K5,
pack kernel and O fix-up against tests/masked_oracle.py on the goldens
tests/golden/m*.npz, at the tolerances of tests/test_gpu_parity.py
(tests/masked_cases.py: which golden is held to what, and why)."""
import numpy as np
import pytest

import masked_cases as mc
import masked_oracle as mo
from conftest import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


def solve(tritd, g, observed="golden", **kw):
    obs = g["observed"] if isinstance(observed, str) else observed
    return tritd.triple_decomp_ADMM(g["D"], g["r"], kw.pop("opts", g["opts"]), g["A0"], g["B0"], g["C0"],
                                    return_E=True, return_iters=True, observed=obs, **kw)


def check_masked(orc, got, g, name, what=""):
    """The comparisons of test_gpu_parity.check_solution on the quantities the
    golden is held to, each figure printed before it is asserted; O and E must
    be exactly 0 at every unobserved entry."""
    A, B, C, O, eh, E, k = got
    held = mc.held(name)
    model = g["opts"].get("model", "cp")
    normD = float(np.linalg.norm(np.where(g["observed"], g["D"], 0.0).ravel()))
    fig = dict(k=k, L=rel(orc.triple_product(A, B, C, model),
                          orc.triple_product(g["A"], g["B"], g["C"], model)))
    if "O" in held:
        fig["O"], fig["E"] = rel(O, g["O"]), rel(E, g["E"])
    else:  # ||O|| is small on this case: against ||Omega o D||
        fig["O"] = float(np.linalg.norm((O - g["O"]).ravel()) / normD)
        fig["E"] = float(np.linalg.norm((E - g["E"]).ravel()) / normD)
    for key, X in (("A", A), ("B", B), ("C", C)):
        fig[key] = rel(X, g[key])
    n = min(len(eh), len(g["errHist"]))
    fig["errHist"] = float(np.max(np.abs(eh[:n] - g["errHist"][:n]) /
                                  (mc.TOL_ERR * np.abs(g["errHist"][:n]) + mc.ATOL_ERR)))
    print(name, what, " ".join("%s=%.2e" % kv for kv in fig.items()))
    assert k == g["k"] and len(eh) == g["k"]
    assert fig["L"] <= mc.TOL_LOE
    assert fig["O"] <= mc.TOL_LOE
    assert fig["E"] <= mc.TOL_LOE
    if "ABC" in held:
        for key in "ABC":
            assert fig[key] <= mc.TOL_ABC, key
    np.testing.assert_allclose(eh, g["errHist"], rtol=mc.TOL_ERR, atol=mc.ATOL_ERR)
    miss = ~g["observed"]
    assert not O[miss].any() and not E[miss].any()


# --- 1. parity ---------------------------------------------------------------
@pytest.mark.parametrize("name", mc.names())
def test_masked_admm_matches_golden(tritd, orc, name):
    g = mc.load(name)
    check_masked(orc, solve(tritd, g), g, name)


@pytest.mark.parametrize("name", [n for n in mc.names() if "it12" in mc.held(n)])
def test_masked_first_iterations(tritd, name):
    g = mc.load(name)
    for it in (1, 2):
        A, B, C, O, eh, E, k = solve(tritd, g, opts=dict(g["opts"], maxIter=it))
        assert k == it
        for key, X in (("A", A), ("B", B), ("C", C)):
            d = rel(X, g[f"it{it}_{key}"])
            print(name, it, key, "%.2e" % d)
            assert d <= mc.TOL_IT12, (it, key)


# --- 2. storage forms ----------------------------------------------------------
@pytest.mark.parametrize("name,env", [
    ("m12x10x8_r2", {"TRITD_DENSE_E": "1"}), ("m12x10x8_r2_stop", {"TRITD_DENSE_E": "1"}),
    ("m30_r3_tile", {"TRITD_DENSE_E": "1"}), ("m17x16x20_r8", {"TRITD_DENSE_E": "1"}),
    ("m19x21x23_r7", {"TRITD_DENSE_E": "1"}), ("m20x24x18_r5_video", {"TRITD_DENSE_E": "1"}),
    ("m54x4x96_r5_sensor", {"TRITD_DENSE_E": "1"}),
    ("m20x6x70_r3", {"TRITD_K5_TSPLIT": "1"}), ("m20x6x70_r3", {"TRITD_K5_TSPLIT": "2"}),
    ("m20x6x70_r3", {"TRITD_K5_TSPLIT": "3"}), ("m30_r3_tile", {"TRITD_K5_TSPLIT": "2"}),
    ("m54x4x96_r5_sensor", {"TRITD_K5_TSPLIT": "3"}),
    ("m20x6x70_r3", {"TRITD_K5_TSPLIT": "3", "TRITD_DENSE_E": "1"}),
    ("mqi12x10x8_r2", {"TRITD_K5_TSPLIT": "2"}),
])
def test_masked_storage_forms_match_golden(tritd, orc, name, env, monkeypatch):
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    g = mc.load(name)
    check_masked(orc, solve(tritd, g), g, name, str(env))
    if "TRITD_DENSE_E" in env:  # the form really ran
        n1, n2, n3 = g["D"].shape
        s = tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3, D=g["D"],
                          device=0, probe=False, observed=g["observed"])
        s.run(1)
        s.sync()
        assert s.k5_profile() == (7, 0) and s.mask_info()[0]
        s.close()


# --- 3. oracle-free invariants -------------------------------------------------
INVARIANT_CASES = ["m12x10x8_r2_stop", "m17x16x20_r8", "m24x20x18_r12", "m20x6x70_r3", "mqi12x10x8_r2"]


def _short(g, iters=12):
    return dict(g["opts"], maxIter=min(iters, g["opts"]["maxIter"]))


@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_all_true_mask_is_the_unmasked_call_bitwise(tritd, name):
    g = mc.load(name)
    opts = _short(g)
    ref = solve(tritd, g, observed=None, opts=opts)
    got = solve(tritd, g, observed=np.ones(g["D"].shape, dtype=bool), opts=opts)
    assert got[6] == ref[6]
    for a, b in zip(got[:6], ref[:6]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_fill_values_never_enter(tritd, name):
    g = mc.load(name)
    opts = _short(g)
    ref = solve(tritd, g, opts=opts)
    for fill in (np.nan, 0.0, 1e30):
        D = g["D"].copy(order="F")
        D[~g["observed"]] = fill
        got = solve(tritd, dict(g, D=D), opts=opts)
        assert got[6] == ref[6]
        for a, b in zip(got[:6], ref[:6]):
            np.testing.assert_array_equal(a, b)


def test_unobserved_zero_after_the_switch_to_dense_e(tritd, synth):
    """lambda = 2e-3 std(D) makes E dense from the first iterations, so the
    session switches to the dense-E K5 after iteration 8 (solver.cpp
    maybe_dense_e): O and E stay exactly 0 where nothing was observed."""
    d = synth.video_like(24, 20, 40, 3)
    observed = np.random.default_rng(5).random(d["D"].shape) >= 0.2
    observed[:16, 1, 16:32] = False
    opts = dict(synth.VIDEO_OPTS, maxIter=12, **{"lambda": 2e-3 * float(np.std(d["D"]))})
    s = tritd.Session(3, opts, d["A0"], d["B0"], d["C0"], n1=24, n2=20, n3=40, D=d["D"], device=0,
                      probe=False, observed=observed)
    try:
        s.run(12)
        res = s.get()
        assert res["k"] == 12
        assert s.k5_profile() == (7, 0), "the session did not switch to dense E"
        assert np.count_nonzero(res["E"]) >= 0.2 * observed.sum()
        assert not res["O"][~observed].any() and not res["E"][~observed].any()
        assert np.isfinite(res["errHist"]).all()
    finally:
        s.close()


def test_mask_info_reports_the_observed_count(tritd):
    g = mc.load("m19x21x23_r7")
    n1, n2, n3 = g["D"].shape
    kw = dict(n1=n1, n2=n2, n3=n3, D=g["D"], device=0, probe=False)
    s = tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], observed=g["observed"], **kw)
    assert s.mask_info() == (True, int(g["observed"].sum()))
    s.close()
    s = tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], **kw)
    assert s.mask_info() == (False, n1 * n2 * n3)
    s.close()


# --- 4. shards -----------------------------------------------------------------
@pytest.mark.parametrize("name,P,serial", [("m30_r3_tile", 2, False), ("m30_r3_tile", 3, False),
                                           ("m19x21x23_r7", 2, False), ("m19x21x23_r7", 3, False),
                                           ("m19x21x23_r7", 2, True)])
def test_masked_device_set_matches_golden(tritd, orc, name, P, serial, monkeypatch):
    """Mode-1 shards: one GPU repeated P times (tritd_set_devices), each shard
    a session with its rows of the mask; TRITD_SHOV=0: the phase-serial order."""
    if serial:
        monkeypatch.setenv("TRITD_SHOV", "0")
    g = mc.load(name)
    tritd.set_devices([0] * P)
    try:
        got = solve(tritd, g)
    finally:
        tritd.set_devices([])
    check_masked(orc, got, g, name, "P=%d" % P)


def test_session_with_device_mask_and_padded_leading_dimension(tritd, orc):
    """D and the mask resident on the device, ldD > n1 (elements of D, bytes
    of the mask), the padding rows holding NaN / nonzero bytes."""
    from tritd import hip
    name = "m19x21x23_r7"
    g = mc.load(name)
    n1, n2, n3 = g["D"].shape
    ld = n1 + 5
    Dp = np.full((ld, n2, n3), np.nan, order="F")
    Dp[:n1] = g["D"]
    Mp = np.full((ld, n2, n3), 0xFF, dtype=np.uint8, order="F")
    Mp[:n1] = g["observed"]
    dD, dM = hip.DeviceArray.from_host(Dp), hip.DeviceArray.from_host(Mp)
    try:
        s = tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3,
                          d_device_ptr=dD.ptr, ldD=ld, device=0, probe=False, observed=dM.ptr)
    finally:
        dD.free()
        dM.free()
    try:
        assert s.mask_info() == (True, int(g["observed"].sum()))
        s.run(g["opts"]["maxIter"])
        r = s.get()
    finally:
        s.close()
    check_masked(orc, (r["A"], r["B"], r["C"], r["O"], r["errHist"], r["E"], r["k"]), g, name, "device")


# --- 5. the payoff -------------------------------------------------------------
@pytest.fixture(scope="module")
def sensor_completion(synth):
    """sensor_like(54,4,96,5), 10 % missing, 100 iterations: the driver's
    inputs and the masked oracle's RRE of L against the clean tensor."""
    from tritd import drivers
    d = synth.sensor_like(54, 4, 96, 5, missing=0.0)
    mask = drivers.missing_mask(d["X"].shape, 0.10, np.random.default_rng(0))
    Y = np.array(d["X"], order="F", copy=True)
    Y[mask] = 0.0
    opts = dict(synth.TRAFFIC_OPTS)
    A, B, C, *_ = mo.triple_decomp_ADMM_masked(Y, ~mask, 5, opts, d["A0"], d["B0"], d["C0"])
    import tritd_oracle
    return d, opts, mo.rre(tritd_oracle.triple_product(A, B, C), d["X"])


def test_traffic_driver_with_the_mask(tritd, sensor_completion):
    from tritd import drivers
    d, opts, rre_oracle = sensor_completion
    kw = dict(r=5, missing_ratio=0.10, opts=opts, seed=0, A0=d["A0"], B0=d["B0"], C0=d["C0"],
              printer=lambda s: None)
    masked = drivers.traffic_triple(d["X"], use_mask=True, **kw)
    filled = drivers.traffic_triple(d["X"], use_mask=False, **kw)
    print("RRE masked %.6e oracle %.6e zero-filled %.6e" % (masked["nrmse"], rre_oracle, filled["nrmse"]))
    assert abs(masked["nrmse"] - rre_oracle) <= 1e-6
    assert masked["nrmse"] < 0.5 * filled["nrmse"]
    assert not masked["O"][masked["mask"]].any()


def test_video_driver_with_the_mask(tritd, synth):
    from tritd import drivers
    d = synth.video_like(20, 24, 18, 3)
    kw = dict(r=3, missing_ratio=0.2, opts=dict(synth.VIDEO_OPTS, maxIter=30), seed=1, A0=d["A0"],
              B0=d["B0"], C0=d["C0"], printer=lambda s: None)
    masked = drivers.video_triple(d["X"], use_mask=True, **kw)
    filled = drivers.video_triple(d["X"], use_mask=False, **kw)
    print("video NRMSE on the missing entries: masked %.3e zero-filled %.3e" % (masked["nrmse"], filled["nrmse"]))
    assert not masked["O"][masked["mask"]].any()
    assert masked["nrmse"] < filled["nrmse"]


# --- 6. refusals ---------------------------------------------------------------
def test_refusals(tritd):
    from tritd import _lib
    g = mc.load("m12x10x8_r2")
    kw = dict(n1=12, n2=10, n3=8, device=0, probe=False)
    with pytest.raises(tritd.TritdError) as e:
        tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], D=g["D"].astype(np.float32),
                      observed=g["observed"], **kw)
    assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED
    none = np.zeros(g["D"].shape, dtype=bool)
    with pytest.raises(tritd.TritdError) as e:
        solve(tritd, g, observed=none)
    assert e.value.status == _lib.TRITD_ERR_ARG
    with pytest.raises(tritd.TritdError) as e:
        tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], D=g["D"], observed=none, **kw)
    assert e.value.status == _lib.TRITD_ERR_ARG
    # the library still solves afterwards
    A, B, C, O, eh, E, k = solve(tritd, g, opts=dict(g["opts"], maxIter=3))
    assert k == 3 and np.isfinite(eh).all()
