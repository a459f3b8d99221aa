"""GPU tests of the mask-aware ALS (observed=): libtritd's masked fit kernel,
which selects X~ = where(Omega, X, Xhat), sums the residual over the observed
entries and writes the TX copy of X~ for the mode-3 contraction, against
tests/masked_als_oracle.py on the goldens tests/golden/oals*.npz, at the
tolerances of tests/test_gpu_als.py (tests/masked_als_cases.py: which golden
is held to what, and why)."""
import numpy as np
import pytest

import masked_als_cases as mac
import masked_als_oracle as mao
from conftest import rel

pytestmark = pytest.mark.gpu

# one golden per padded rank (16, 32, 48, 64) plus the special tiles and the 5 t-tiles
INVARIANT_CASES = ["oals12x10x8_r2_stop", "oals21x13x35_r5", "oals18x19x22_r6", "oals17x16x20_r8",
                   "oals30_r3_tiles", "oals20x6x70_r3"]


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
    return tritd.triple_decomp_ALS(g["X"], g["r"], kw.pop("opts", g["opts"]), g["A0"], g["B0"], g["C0"],
                                   return_iters=True, observed=obs, **kw)


def check_masked(orc, got, g, name, what=""):
    """The comparisons of test_gpu_als.check on the quantities the golden is
    held to, each figure printed before it is asserted."""
    A, B, C, eh, k = got
    held = mac.held(name)
    fig = dict(k=k, L=rel(orc.triple_product(A, B, C), orc.triple_product(g["A"], g["B"], g["C"])))
    for key, X in (("A", A), ("B", B), ("C", C)):
        fig[key] = rel(X, g[key])
    n = min(len(eh), len(g["errHist"]))
    fig["errHist"] = float(np.max(np.abs(eh[:n] - g["errHist"][:n]) / np.abs(g["errHist"][:n])))
    print(name, what, " ".join("%s=%.2e" % kv for kv in fig.items()))
    assert k == g["k"] and len(eh) == g["k"]
    np.testing.assert_allclose(eh, g["errHist"], rtol=mac.TOL_ERR, atol=mac.ATOL_ERR)
    assert fig["L"] <= mac.TOL_L
    if "ABC" in held:
        for key in "ABC":
            assert fig[key] <= mac.TOL_ABC, key


def same(got, ref):
    assert got[4] == ref[4]
    for a, b in zip(got[:4], ref[:4]):
        np.testing.assert_array_equal(a, b)


# --- 1. parity ---------------------------------------------------------------
@pytest.mark.parametrize("name", mac.names())
def test_masked_als_matches_golden(tritd, orc, name):
    g = mac.load(name)
    check_masked(orc, solve(tritd, g), g, name)


def test_stop_golden_returns_the_factors_un_updated(tritd, orc):
    """The stop test fires before maxIter; errHist(k) is the error of the
    returned factors on the observed entries (they were not updated after it)."""
    g = mac.load("oals12x10x8_r2_stop")
    A, B, C, eh, k = solve(tritd, g)
    assert k == g["k"] < g["opts"]["maxIter"]
    Xo = np.where(g["observed"], g["X"], 0.0)
    e = np.linalg.norm(np.where(g["observed"], Xo - orc.triple_product(A, B, C), 0.0).ravel()) / \
        np.linalg.norm(Xo.ravel())
    assert abs(e - eh[-1]) <= 1e-12 * eh[-1]


# --- 2, 3. oracle-free invariants ----------------------------------------------
@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_all_true_mask_is_the_unmasked_call_bitwise(tritd, name):
    g = mac.load(name)
    ref = solve(tritd, g, observed=None)
    same(solve(tritd, g, observed=np.ones(g["X"].shape, dtype=bool)), ref)


@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_fill_values_never_enter(tritd, name):
    g = mac.load(name)
    ref = solve(tritd, dict(g, X=np.where(g["observed"], g["X"], 0.0)))
    assert np.isfinite(ref[3]).all()
    for fill in (np.nan, np.inf, -1e30):
        X = g["X"].copy(order="F")
        X[~g["observed"]] = fill
        same(solve(tritd, dict(g, X=X)), ref)


# --- 4. session -----------------------------------------------------------------
def session(tritd, g, **kw):
    n1, n2, n3 = g["X"].shape
    return tritd.AlsSession(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3, **kw)


def session_result(s, iters):
    try:
        for it in iters:
            s.run(it)
        r = s.get()
    finally:
        s.close()
    return r["A"], r["B"], r["C"], r["errHist"], r["k"]


@pytest.mark.parametrize("name", ["oals19x21x23_r7", "oals20x6x70_r3"])
def test_session_steps_and_mask_info(tritd, orc, name):
    g = mac.load(name)
    assert g["opts"]["maxIter"] >= 8
    s = session(tritd, g, X=g["X"], observed=g["observed"])
    assert s.mask_info() == (True, int(g["observed"].sum()))
    whole = session_result(s, (8,))
    same(session_result(session(tritd, g, X=g["X"], observed=g["observed"]), (3, 5)), whole)
    if g["opts"]["maxIter"] == 8:
        check_masked(orc, whole, g, name, "session")
    s = session(tritd, g, X=g["X"])
    assert s.mask_info() == (False, g["X"].size)
    s.close()


def test_session_with_device_mask_and_padded_leading_dimension(tritd):
    """X and the mask resident on the device, ldX = n1 + 3 (elements of X,
    bytes of the mask), the padding rows holding NaN / nonzero bytes."""
    from tritd import hip
    g = mac.load("oals19x21x23_r7")
    n1, n2, n3 = g["X"].shape
    iters = (g["opts"]["maxIter"],)
    host = session_result(session(tritd, g, X=g["X"], observed=g["observed"]), iters)
    ld = n1 + 3
    Xp = np.full((ld, n2, n3), np.nan, order="F")
    Xp[:n1] = g["X"]
    Mp = np.full((ld, n2, n3), 0xFF, dtype=np.uint8, order="F")
    Mp[:n1] = g["observed"]
    dX, dM = hip.DeviceArray.from_host(Xp), hip.DeviceArray.from_host(Mp)
    try:
        s = session(tritd, g, x_device_ptr=dX.ptr, ldX=ld, observed=dM.ptr)
    finally:
        dX.free()
        dM.free()
    assert s.mask_info() == (True, int(g["observed"].sum()))
    same(session_result(s, iters), host)


# --- 5. device sets -------------------------------------------------------------
@pytest.mark.parametrize("name,P,serial", [("oals30_r3_tiles", 2, False), ("oals30_r3_tiles", 3, False),
                                           ("oals19x21x23_r7", 2, False), ("oals19x21x23_r7", 3, False),
                                           ("oals30_r3_tiles", 2, True), ("oals19x21x23_r7", 3, True)])
def test_masked_device_set_matches_golden(tritd, orc, name, P, serial, monkeypatch):
    """Mode-1 shards whose boundaries fall inside the 16-row tiles: one GPU
    repeated P times (tritd_set_devices), each shard a session with its rows
    of the mask; TRITD_SHOV=0: the phase-serial order."""
    if serial:
        monkeypatch.setenv("TRITD_SHOV", "0")
    g = mac.load(name)
    assert any((g["X"].shape[0] * p // P) % 16 for p in range(1, P))
    tritd.set_devices([0] * P)
    try:
        got = solve(tritd, g)
    finally:
        tritd.set_devices([])
    check_masked(orc, got, g, name, "P=%d%s" % (P, " serial" if serial else ""))


# --- 6. refusals ----------------------------------------------------------------
def test_refusals(tritd):
    from tritd import _lib
    g = mac.load("oals12x10x8_r2")
    none = np.zeros(g["X"].shape, dtype=bool)
    with pytest.raises(tritd.TritdError) as e:
        solve(tritd, g, observed=none)
    assert e.value.status == _lib.TRITD_ERR_ARG
    with pytest.raises(tritd.TritdError) as e:
        session(tritd, g, X=g["X"], observed=none)
    assert e.value.status == _lib.TRITD_ERR_ARG
    for serial in (False, True):
        # a device set: every shard refuses alike ...
        tritd.set_devices([0, 0])
        try:
            with pytest.MonkeyPatch.context() as mp:
                if serial:
                    mp.setenv("TRITD_SHOV", "0")
                with pytest.raises(tritd.TritdError) as e:
                    solve(tritd, g, observed=none)
                assert e.value.status == _lib.TRITD_ERR_ARG
                # ... and one shard (rows 0..5) without an observed entry beside one with some still solves
                half = g["observed"].copy(order="F")
                half[:6] = False
                A, B, C, eh, k = solve(tritd, g, observed=half)
                assert k == g["opts"]["maxIter"] and np.isfinite(eh).all() and np.isfinite(A).all()
        finally:
            tritd.set_devices([])
    with pytest.raises(ValueError, match="observed must have the shape of X"):
        solve(tritd, g, observed=g["observed"][:, :-1])
    with pytest.raises(ValueError, match=r"set_devices\(\[d\] \* P\)"):
        solve(tritd, g, virtual_shards=2)
    # the library still solves an unmasked ALS afterwards
    A, B, C, eh, k = solve(tritd, g, observed=None, opts=dict(maxIter=3, tol=0.0))
    assert k == 3 and np.isfinite(eh).all()


# --- 7. the payoff --------------------------------------------------------------
def test_masked_fit_beats_zero_fill_on_the_missing_entries(tritd):
    d, observed, r, opts = mac.completion_case()
    args = (r, opts, d["A0"], d["B0"], d["C0"])
    A, B, C, eh = tritd.triple_decomp_ALS(d["X"], *args, observed=observed)
    masked = mao.missing_error(A, B, C, d["Lstar"], observed)
    A, B, C, _ = tritd.triple_decomp_ALS(np.where(observed, d["X"], 0.0), *args)
    filled = mao.missing_error(A, B, C, d["Lstar"], observed)
    print("relative error on the missing entries: masked %.3e zero-filled %.3e" % (masked, filled))
    assert np.isfinite(eh).all()
    assert masked < filled
