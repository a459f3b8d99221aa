"""GPU tests of the mask-aware nonconvex solver (observed=): libtritd's
k_als_fit<RP, true, true>, which selects X~ = where(Omega, X, T), runs the
outlier chain of test.m:36-48 on it with the unobserved values imposed, and
writes the TX copy of X~ for the mode-3 contraction, against
tests/masked_ncvx_oracle.py: the goldens tests/golden/onc*.npz, the rank sweep
r = 1..8, the bitwise invariants, device sets, and the steppable session
(tritd_als_session_set_ncvx / tritd_als_session_get_O).  Tolerances are those
of tests/test_ncvx.py (tests/masked_ncvx_cases.py)."""
import numpy as np
import pytest

import masked_ncvx_cases as mnc
import masked_ncvx_oracle as mno
import masked_sweep_cases as msc
from conftest import rel

pytestmark = pytest.mark.gpu

# one case per padded rank (16, 32, 48, 64) of the rank sweep
RANK_PER_FORM = (3, 5, 6, 8)


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    t.set_printer(lambda s: None)
    yield t
    t.set_printer(None)


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


def solve(tritd, g, observed="golden", X=None, **over):
    obs = g["observed"] if isinstance(observed, str) else observed
    return tritd.triple_decomp_ncvx(g["X"] if X is None else X, g["r"], *mnc.args(g, **over), g["A0"],
                                    g["B0"], g["C0"], return_iters=True, observed=obs)


def sweep_golden(r, hidden=0):
    """The sweep inputs and their reference in the form of a golden."""
    c = mnc.sweep_inputs(r, msc.hidden_shard_mask(("cp", r), hidden) if hidden else None)
    prm = mnc.sweep_args()
    g = dict(X=c["D"], observed=c["observed"], r=r, A0=c["A0"], B0=c["B0"], C0=c["C0"],
             opts=dict(zip(mnc.PARAM_KEYS, prm)))
    g.update(mnc.sweep_reference(r, hidden))
    return g


def check(orc, got, g, what, trace=None):
    """A, B, C, O, triple_product <= 1e-9, errHist rtol 1e-8 / atol 1e-13, same
    k; every figure printed before it is asserted."""
    A, B, C, O, eh, k = got
    ref = dict(A=g["A"], B=g["B"], C=g["C"], O=g["O"]) if trace is None else \
        {key: g["it%d_%s" % (trace, key)] for key in "ABCO"}
    fig = dict(k=k, L=rel(orc.triple_product(A, B, C), orc.triple_product(ref["A"], ref["B"], ref["C"])))
    for key, X in (("A", A), ("B", B), ("C", C), ("O", O)):
        fig[key] = rel(X, ref[key])
    if trace is None:
        n = min(len(eh), len(g["errHist"]))
        fig["errHist"] = float(np.max(np.abs(eh[:n] - g["errHist"][:n]) / np.abs(g["errHist"][:n])))
    print(what, " ".join("%s=%.2e" % kv for kv in fig.items()), flush=True)
    tol = mnc.TOL if trace is None else mnc.TOL_TRACE
    for key in ("L", "A", "B", "C", "O"):
        assert fig[key] <= tol, key
    if trace is None:
        assert k == g["k"] and len(eh) == len(g["errHist"])
        np.testing.assert_allclose(eh, g["errHist"], rtol=mnc.RTOL_ERR, atol=mnc.ATOL_ERR)
    else:
        assert k == trace
    assert not O[~g["observed"]].any()


def same(got, ref):
    assert got[5] == ref[5]
    for a, b in zip(got[:5], ref[:5]):
        np.testing.assert_array_equal(a, b)


# --- 1. parity -----------------------------------------------------------------
@pytest.mark.parametrize("name", mnc.names())
def test_masked_ncvx_matches_golden(tritd, orc, name):
    g = mnc.load(name)
    assert set(mnc.held(name)) == set(mnc.DEFAULT)
    check(orc, solve(tritd, g), g, name)


def test_first_two_iterations_and_alias(tritd, orc):
    g = mnc.load("onc12x10x8_r2")
    for it in (1, 2):
        got = tritd.triple_decomp_ADMM_outlier(g["X"], g["r"], *mnc.args(g, maxIter=it), g["A0"], g["B0"],
                                               g["C0"], return_iters=True, observed=g["observed"])
        check(orc, got, g, "onc12x10x8_r2 iteration %d" % it, trace=it)


def test_stop_golden_returns_the_previous_O(tritd):
    g = mnc.load("onc20x24x18_r3_stop")
    got = solve(tritd, g)
    assert got[5] == g["k"] < g["opts"]["maxIter"] and len(got[4]) == g["k"]
    cut = solve(tritd, g, maxIter=g["k"] - 1)
    assert cut[5] == g["k"] - 1
    np.testing.assert_array_equal(got[3], cut[3])


@pytest.mark.parametrize("r", mnc.SWEEP_RANKS)
def test_rank_sweep(tritd, orc, r):
    """All four padded ranks, with and without rank padding, ragged tiles in
    every mode, a wholly missing tile, an edge tile with no observed real row
    and a fully observed tile (tests/masked_sweep_cases.py)."""
    g = sweep_golden(r)
    assert np.count_nonzero(g["O"]) > 0
    check(orc, solve(tritd, g), g, "masked ncvx sweep r=%d" % r)


# --- 2. bitwise invariants -----------------------------------------------------
@pytest.mark.parametrize("r", RANK_PER_FORM)
def test_all_true_mask_is_the_unmasked_call_bitwise(tritd, r):
    g = sweep_golden(r)
    assert mnc.padded_rank(r) == {3: 16, 5: 32, 6: 48, 8: 64}[r]
    ref = solve(tritd, g, observed=None)
    assert np.count_nonzero(ref[3]) > 0
    same(solve(tritd, g, observed=np.ones(g["X"].shape, dtype=bool)), ref)


@pytest.mark.parametrize("r", RANK_PER_FORM)
def test_fill_values_never_enter_and_O_is_zero_where_unobserved(tritd, r):
    g = sweep_golden(r)
    U = ~g["observed"]
    ref = solve(tritd, g, X=np.where(g["observed"], g["X"], 0.0))
    assert np.isfinite(ref[4]).all() and np.isfinite(ref[3]).all()
    assert not ref[3][U].any() and ref[3][~U].any()
    for fill in (np.nan, np.inf, -1e30):
        X = g["X"].copy(order="F")
        X[U] = fill
        same(solve(tritd, g, X=X), ref)


def test_O_is_zero_where_unobserved_with_lambda_zero(tritd):
    """lambda = 0: the soft threshold keeps every residue, so an O_new left to
    the rounding of (T + rho T)/(1 + rho) would be nonzero at missing entries."""
    g = sweep_golden(3)
    A, B, C, O, eh, k = solve(tritd, g, **{"lambda": 0.0, "maxIter": 3})
    assert not O[~g["observed"]].any() and O[g["observed"]].any()


# --- 3. device sets and sharding -------------------------------------------------
@pytest.mark.parametrize("serial", [False, True])
def test_device_set_matches_golden(tritd, orc, serial, monkeypatch):
    """Mode-1 shards (10 rows each: boundaries inside the 16-row tiles) on one
    GPU repeated; TRITD_SHOV=0: the phase-serial order."""
    if serial:
        monkeypatch.setenv("TRITD_SHOV", "0")
    g = mnc.load("onc30_r3_tiles")
    tritd.set_devices([0, 0, 0])
    try:
        got = solve(tritd, g)
    finally:
        tritd.set_devices([])
    check(orc, got, g, "onc30_r3_tiles set_devices([0,0,0])%s" % (" TRITD_SHOV=0" if serial else ""))


def test_a_shard_with_nothing_observed(tritd, orc):
    g = sweep_golden(3, hidden=3)
    H = g["observed"]
    assert not H[:H.shape[0] // 3].any() and H[H.shape[0] // 3:].any()
    tritd.set_devices([0, 0, 0])
    try:
        got = solve(tritd, g)
    finally:
        tritd.set_devices([])
    check(orc, got, g, "hidden shard, set_devices([0,0,0])")


def test_all_false_mask_is_refused_everywhere(tritd):
    from tritd import _lib
    g = mnc.load("onc12x10x8_r2")
    none = np.zeros(g["X"].shape, dtype=bool)
    with pytest.raises(tritd.TritdError) as e:
        solve(tritd, g, observed=none)
    assert e.value.status == _lib.TRITD_ERR_ARG
    for serial in (False, True):
        tritd.set_devices([0, 0, 0])
        try:
            with pytest.MonkeyPatch.context() as mp:
                if serial:
                    mp.setenv("TRITD_SHOV", "0")
                with pytest.raises(tritd.TritdError) as e:
                    solve(tritd, g, observed=none)
                assert e.value.status == _lib.TRITD_ERR_ARG
        finally:
            tritd.set_devices([])
    with pytest.raises(tritd.TritdError) as e:
        session(tritd, g, X=g["X"], observed=none)
    assert e.value.status == _lib.TRITD_ERR_ARG
    # the library still solves afterwards
    A, B, C, O, eh, k = solve(tritd, g, observed=None, maxIter=3)
    assert k == 3 and np.isfinite(eh).all() and np.isfinite(O).all()


# --- 4. sessions ---------------------------------------------------------------------
def session(tritd, g, ncvx="golden", maxIter=8, **kw):
    n1, n2, n3 = g["X"].shape
    if isinstance(ncvx, str):
        ncvx = mnc.ncvx_dict(mnc.args(g))
    return tritd.AlsSession(g["r"], dict(maxIter=maxIter, tol=g["opts"]["tol"]), g["A0"], g["B0"], g["C0"],
                            n1=n1, n2=n2, n3=n3, ncvx=ncvx, **kw)


def session_result(s, iters):
    try:
        for it in iters:
            s.run(it)
        r = s.get()
        O = s.get_O()
    finally:
        s.close()
    return r["A"], r["B"], r["C"], O, r["errHist"], r["k"]


@pytest.mark.parametrize("name", ["onc20x6x70_r3", "onc30_r3_tiles"])
def test_session_steps_equal_the_one_shot_call(tritd, name):
    g = mnc.load(name)
    whole = solve(tritd, g, maxIter=8)
    assert whole[5] == 8
    s = session(tritd, g, X=g["X"], observed=g["observed"])
    assert s.mask_info() == (True, int(g["observed"].sum()))
    same(session_result(s, (3, 5)), whole)


def test_session_with_device_mask_and_padded_leading_dimension(tritd):
    """X and the mask resident on the device, ldX = n1 + 5 (elements of X,
    bytes of the mask), the padding rows holding NaN / nonzero bytes."""
    from tritd import hip
    g = mnc.load("onc20x6x70_r3")
    n1, n2, n3 = g["X"].shape
    whole = solve(tritd, g, maxIter=8)
    ld = n1 + 5
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
    same(session_result(s, (3, 5)), whole)


def test_session_with_a_one_rank_communicator(tritd):
    g = mnc.load("onc30_r3_tiles")
    whole = solve(tritd, g, maxIter=8)
    comm = tritd.Comm(tritd.Comm.unique_id(), 1, 0, 0)
    try:
        got = session_result(session(tritd, g, X=g["X"], observed=g["observed"], comm=comm), (3, 5))
    finally:
        comm.close()
    same(got, whole)


def test_unmasked_session_equals_the_one_shot_call(tritd):
    g = mnc.load("onc20x6x70_r3")
    whole = solve(tritd, g, observed=None, maxIter=8)
    s = session(tritd, g, X=g["X"])
    assert s.mask_info() == (False, g["X"].size)
    same(session_result(s, (3, 5)), whole)


def test_session_stop_returns_the_previous_O(tritd):
    g = mnc.load("onc20x24x18_r3_stop")
    whole = solve(tritd, g)
    s = session(tritd, g, X=g["X"], observed=g["observed"], maxIter=g["opts"]["maxIter"])
    s.run(g["opts"]["maxIter"])
    assert s.sync() == (g["k"], True)
    same(session_result(s, ()), whole)


def test_session_call_order(tritd):
    from tritd import _lib
    g = mnc.load("onc12x10x8_r2")
    prm = mnc.args(g)[:6]
    s = session(tritd, g, ncvx=None, X=g["X"], observed=g["observed"])
    try:
        with pytest.raises(tritd.TritdError) as e:   # a plain ALS session has no O
            s.get_O()
        assert e.value.status == _lib.TRITD_ERR_STATE
        s.run(1)
        with pytest.raises(tritd.TritdError) as e:   # set_ncvx comes before the first run
            s.set_ncvx(*prm)
        assert e.value.status == _lib.TRITD_ERR_STATE
        assert s.get()["k"] == 1                     # and the ALS session goes on
    finally:
        s.close()
    s = session(tritd, g, ncvx=None, X=g["X"])
    try:
        with pytest.raises(tritd.TritdError) as e:
            s.set_ncvx(0.0, *prm[1:])
        assert e.value.status == _lib.TRITD_ERR_ARG
    finally:
        s.close()


# --- 5. progress lines -------------------------------------------------------------
def test_prints_like_the_oracle(tritd):
    g = mnc.load("onc12x10x8_r2")
    prm = mnc.args(g, maxIter=3)
    ref, lines = [], []
    mno.triple_decomp_ncvx_masked(g["X"], g["observed"], g["r"], *prm, g["A0"], g["B0"], g["C0"],
                                  printer=ref.append)
    tritd.set_printer(lines.append)
    try:
        tritd.triple_decomp_ncvx(g["X"], g["r"], *prm, g["A0"], g["B0"], g["C0"], observed=g["observed"])
    finally:
        tritd.set_printer(lambda s: None)
    assert len(ref) == 3 and lines == ref


# --- 6. the payoff -----------------------------------------------------------------
def test_masked_fit_beats_zero_fill_on_the_missing_entries(tritd):
    d, observed, r, prm = mnc.completion_case()
    args = (r, *prm, d["A0"], d["B0"], d["C0"])
    A, B, C, O, eh = tritd.triple_decomp_ncvx(d["X"], *args, observed=observed)
    masked = mno.missing_error(A, B, C, d["Lstar"], observed)
    A, B, C, _, _ = tritd.triple_decomp_ncvx(np.where(observed, d["X"], 0.0), *args)
    filled = mno.missing_error(A, B, C, d["Lstar"], observed)
    print("relative error on the missing entries: masked %.3e zero-filled %.3e" % (masked, filled))
    assert np.isfinite(eh).all()
    assert masked <= mnc.COMPLETION_MAX
    assert mnc.COMPLETION_GAIN * masked <= filled
