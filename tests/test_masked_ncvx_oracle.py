"""CPU tests of the mask-aware nonconvex solver: the masked oracle
(tests/masked_ncvx_oracle.py) against its goldens and against the unmasked
oracle, the admission rule of the goldens and of the rank sweep, and what the
new entry points promise without a device."""
import inspect

import numpy as np
import pytest

import masked_ncvx_cases as mnc
import masked_ncvx_oracle as mno
import tritd_oracle as orc
from conftest import golden_names, load_golden, rel

quiet = mnc.quiet


def run(g, observed="golden", X=None, trace_iters=(), **over):
    obs = g["observed"] if isinstance(observed, str) else observed
    return mno.triple_decomp_ncvx_masked(g["X"] if X is None else X, obs, g["r"],
                                         *mnc.args(g, **over), g["A0"], g["B0"], g["C0"],
                                         printer=quiet, trace_iters=trace_iters)


def same(got, ref, n=5):
    assert got[5] == ref[5]
    for a, b in zip(got[:n], ref[:n]):
        np.testing.assert_array_equal(a, b)


@pytest.fixture(scope="module")
def reruns():
    """The oracle rerun on every golden's inputs, once (iterations 1 and 2 traced)."""
    return {name: (g, run(g, trace_iters=(1, 2))) for name, g in ((n, mnc.load(n)) for n in mnc.names())}


def test_goldens_present():
    assert mnc.names() == ["onc12x10x8_r2", "onc20x24x18_r3_stop", "onc20x6x70_r3", "onc30_r3_tiles"]
    assert mnc.load("onc20x6x70_r3")["X"].shape == (20, 6, 70)  # five t-tiles
    # none of the patterns the other suites glob matches the new files
    for kind in ("admm", "qi", "als", "ncvx"):
        assert not set(golden_names(kind)) & set(mnc.names())


@pytest.mark.parametrize("name", mnc.names())
def test_oracle_reproduces_golden(reruns, name):
    g, (A, B, C, O, eh, k, tr) = reruns[name]
    assert k == g["k"] and len(eh) == len(g["errHist"])
    for key, X in (("A", A), ("B", B), ("C", C), ("O", O)):
        assert rel(X, g[key]) <= 1e-12, key
    np.testing.assert_allclose(eh, g["errHist"], rtol=1e-12, atol=1e-15)
    for it in (1, 2):
        if "it%d_A" % it in g:
            for key in ("A", "B", "C", "O", "Lam", "Gam"):
                assert rel(tr[it][key], g["it%d_%s" % (it, key)]) <= 1e-12, (it, key)
    assert "it2_O" in mnc.load("onc12x10x8_r2")


@pytest.mark.parametrize("name", mnc.names())
def test_golden_admission_rule(name):
    """Every tolerance a golden is held to is at least 100x its stored drift,
    and the perturbed reruns stopped at the same k."""
    g = mnc.load(name)
    assert float(g["drift_k"]) == 0.0
    assert set(mnc.held(name)) == set(mnc.DEFAULT)
    for q in mnc.held(name):
        key, tol = mnc.QUANTITIES[q]
        assert mnc.MARGIN * float(g[key]) <= tol, (q, float(g[key]), tol)
    assert (~g["observed"]).any() and g["observed"].any()
    assert np.count_nonzero(g["O"]) > 0


def test_golden_inputs_are_those_of_the_unmasked_goldens():
    for name, src in (("onc12x10x8_r2", "nc12x10x8_r2"), ("onc20x24x18_r3_stop", "nc20x24x18_r3_stop"),
                      ("onc30_r3_tiles", "nc30_r3")):
        g, u = mnc.load(name), load_golden(src)
        for key in ("X", "A0", "B0", "C0"):
            np.testing.assert_array_equal(g[key], u[key])
        assert g["r"] == u["r"]
    W = mnc.load("onc20x24x18_r3_stop")["observed"]
    np.testing.assert_array_equal(W, np.random.default_rng(5).random(W.shape) >= 0.15)


def test_tiles_golden_has_the_three_special_tiles():
    obs = mnc.load("onc30_r3_tiles")["observed"]
    assert obs.shape[0] == 30
    assert obs[:16, 1, 16:32].sum() == 0      # a wholly missing 16 x 16 tile
    assert obs[16:, 2, :16].sum() == 0        # a ragged edge tile with no observed real row
    assert obs[:16, 3, :16].all()             # a fully observed tile


@pytest.mark.parametrize("name", golden_names("ncvx"))
def test_all_true_mask_is_the_reference_bitwise(name):
    g = load_golden(name)
    ref = orc.triple_decomp_ADMM_ncvx(g["X"], g["r"], *mnc.args(g), g["A0"], g["B0"], g["C0"],
                                      printer=quiet)
    for observed in (None, np.ones(g["X"].shape, dtype=bool)):
        same(run(g, observed=observed), ref)


@pytest.mark.parametrize("name", mnc.names())
def test_unobserved_state_is_zero_and_fill_values_never_enter(reruns, name):
    g, ref = reruns[name]
    U = ~g["observed"]
    assert not ref[3][U].any()
    for it in (1, 2):
        for key in ("O", "Lam", "Gam"):
            assert not ref[6][it][key][U].any(), (it, key)
    assert np.isfinite(ref[4]).all()
    for fill in (np.nan, np.inf, -1e30):
        X = g["X"].copy(order="F")
        X[U] = fill
        same(run(g, X=X), ref)
    same(run(g, X=np.where(g["observed"], g["X"], 0.0)), ref)


def test_duals_stay_zero_where_unobserved_to_the_last_iteration():
    g = mnc.load("onc20x6x70_r3")
    k = g["k"]
    tr = run(g, trace_iters=(k,))[6][k]
    U = ~g["observed"]
    assert not tr["Lam"][U].any() and not tr["Gam"][U].any() and not tr["O"][U].any()
    assert tr["Lam"][~U].any() and tr["Gam"][~U].any()


def test_stop_golden_stops_early_and_returns_the_previous_O(reruns):
    g, ref = reruns["onc20x24x18_r3_stop"]
    k, tol, eh = g["k"], g["opts"]["tol"], g["errHist"]
    assert 2 < k < g["opts"]["maxIter"] and len(eh) == k
    change = np.abs(np.diff(eh)) / eh[:-1]
    assert change[-1] < tol
    assert (change[:-1] >= 2.0 * tol).all()   # no earlier iteration came near the stop test
    cut = run(g, maxIter=k - 1)
    assert cut[5] == k - 1
    np.testing.assert_array_equal(cut[3], ref[3])   # the returned O is that of iteration k-1
    assert rel(ref[3], g["O"]) <= 1e-12


@pytest.mark.parametrize("r", mnc.SWEEP_RANKS)
def test_sweep_inputs_pass_the_admission_rule_with_an_active_O(r):
    c = mnc.sweep_inputs(r)
    ref = mnc.sweep_reference(r)
    assert ref["k"] == mnc.SWEEP_ITERS
    t = (ref["A"], ref["B"], ref["C"], ref["O"], ref["errHist"], ref["k"])
    dr = mnc.drifts(t, c["D"], c["observed"], r, mnc.sweep_args(), c["A0"], c["B0"], c["C0"])
    active = np.count_nonzero(ref["O"]) / np.count_nonzero(c["observed"])
    print("r=%d nnz(O)/nnz(observed)=%.3f" % (r, active), " ".join("%s=%.1e" % kv for kv in dr.items()))
    assert dr["k"] == 0.0
    for q, (_, tol) in mnc.QUANTITIES.items():
        assert mnc.MARGIN * dr[q] <= tol, (q, dr[q], tol)
    assert mnc.O_ACTIVE_BAND[0] <= active <= mnc.O_ACTIVE_BAND[1]
    assert not ref["O"][~c["observed"]].any()


def test_hidden_shard_inputs_pass_the_admission_rule():
    """The sweep's r = 3 inputs with shard 0 of three observing nothing (the
    GPU suite's device-set case)."""
    import masked_sweep_cases as msc
    H = msc.hidden_shard_mask(("cp", 3), 3)
    c = mnc.sweep_inputs(3, H)
    ref = mnc.sweep_reference(3, 3)
    t = (ref["A"], ref["B"], ref["C"], ref["O"], ref["errHist"], ref["k"])
    dr = mnc.drifts(t, c["D"], H, 3, mnc.sweep_args(), c["A0"], c["B0"], c["C0"])
    print(" ".join("%s=%.1e" % kv for kv in dr.items()))
    assert dr["k"] == 0.0 and ref["k"] == mnc.SWEEP_ITERS
    for q, (_, tol) in mnc.QUANTITIES.items():
        assert mnc.MARGIN * dr[q] <= tol, (q, dr[q], tol)


def test_masked_fit_beats_zero_fill_on_the_missing_entries():
    d, observed, r, prm = mnc.completion_case()
    m = mno.triple_decomp_ncvx_masked(d["X"], observed, r, *prm, d["A0"], d["B0"], d["C0"], printer=quiet)
    z = orc.triple_decomp_ADMM_ncvx(np.where(observed, d["X"], 0.0), r, *prm, d["A0"], d["B0"], d["C0"],
                                    printer=quiet)
    masked = mno.missing_error(*m[:3], d["Lstar"], observed)
    filled = mno.missing_error(*z[:3], d["Lstar"], observed)
    print("relative error on the missing entries: masked %.3e zero-filled %.3e" % (masked, filled))
    assert masked <= mnc.COMPLETION_MAX
    assert mnc.COMPLETION_GAIN * masked <= filled


def test_progress_line_every_iteration():
    g = mnc.load("onc12x10x8_r2")
    lines = []
    eh = mno.triple_decomp_ncvx_masked(g["X"], g["observed"], g["r"], *mnc.args(g, maxIter=4), g["A0"],
                                       g["B0"], g["C0"], printer=lines.append)[4]
    assert lines == ["Iteration %d, relative error = %.4e" % (i, eh[i - 1]) for i in (1, 2, 3, 4)]


# ---------------------------------------------------------------------------
# the new entry points, without a device
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ("tritd_ncvx_masked_f64", "tritd_als_session_set_ncvx", "tritd_als_session_get_O")


def test_new_symbols_are_bound_with_the_documented_signatures():
    import ctypes as C

    import tritd
    from tritd import _lib
    vp, i64 = C.c_void_p, C.c_int64
    sig = {**_lib.SIGNATURES, **_lib.SIGNATURES_MIXED_CASE}
    for name in NEW_SYMBOLS:
        assert name in sig and hasattr(_lib.lib, name)
        assert sig[name][0] is C.c_int
        assert getattr(_lib.lib, name).restype is C.c_int
        assert list(getattr(_lib.lib, name).argtypes) == sig[name][1]
    one = list(sig["tritd_ncvx_f64"][1])
    assert sig["tritd_ncvx_masked_f64"][1] == one[:1] + [vp] + one[1:]
    assert sig["tritd_als_session_set_ncvx"][1] == [vp] + [C.c_double] * 6
    assert sig["tritd_als_session_get_O"][1] == [vp, vp, i64]
    assert inspect.signature(tritd.triple_decomp_ncvx).parameters["observed"].default is None
    assert inspect.signature(tritd.AlsSession.__init__).parameters["ncvx"].default is None
    assert callable(tritd.AlsSession.get_O)


def test_header_declares_the_new_entry_points():
    import os

    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "tritd.h")).read()
    for name in NEW_SYMBOLS:
        assert ("tritd_status %s(" % name) in h
    # and the library exports them
    import subprocess

    from tritd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in NEW_SYMBOLS:
        assert ("T %s\n" % name) in out


def test_observed_shape_mismatch_raises():
    import tritd
    g = mnc.load("onc12x10x8_r2")
    for fn in (tritd.triple_decomp_ncvx, tritd.triple_decomp_ADMM_outlier):
        with pytest.raises(ValueError, match="observed must have the shape of X"):
            fn(g["X"], g["r"], *mnc.args(g), g["A0"], g["B0"], g["C0"], observed=g["observed"][:, :, :-1])
    with pytest.raises(ValueError, match="observed must have the shape of X"):
        tritd.AlsSession(g["r"], dict(maxIter=3, tol=0.0), g["A0"], g["B0"], g["C0"], n1=12, n2=10, n3=8,
                         X=g["X"], observed=g["observed"].ravel(),
                         ncvx=mnc.ncvx_dict(mnc.args(g)))
