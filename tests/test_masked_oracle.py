"""CPU tests of the mask-aware ADMM: the masked oracle against its goldens and
against the unmasked oracle, the admission rule of the goldens, and the
argument errors of the new entry points that need no device."""
import numpy as np
import pytest

import masked_cases as mc
import masked_oracle as mo
import tritd_oracle as orc
from conftest import rel


@pytest.fixture(scope="module")
def reruns():
    """The oracle rerun on every golden's inputs, once."""
    out = {}
    for name in mc.names():
        g = mc.load(name)
        out[name] = (g, mo.triple_decomp_ADMM_masked(g["D"], g["observed"], g["r"], g["opts"],
                                                     g["A0"], g["B0"], g["C0"], trace_iters=(1, 2)))
    return out


def test_goldens_present():
    assert len(mc.names()) >= 10


@pytest.mark.parametrize("name", mc.names())
def test_masked_oracle_reproduces_golden(reruns, name):
    """Another BLAS or thread count reorders sums: a perturbation below the
    1e-15 the stored drift was measured with, so 10x the drift bounds it."""
    g, (A, B, C, O, eh, E, k, tr) = reruns[name]
    assert k == g["k"] and len(eh) == k
    normD = np.linalg.norm(np.where(g["observed"], g["D"], 0.0).ravel())

    def bound(key):
        return 10.0 * max(float(g[key]), 1e-13)

    for key, X in (("A", A), ("B", B), ("C", C)):
        assert rel(X, g[key]) <= bound("drift_ABC"), key
    assert np.linalg.norm((O - g["O"]).ravel()) / normD <= bound("drift_O_normD")
    assert np.linalg.norm((E - g["E"]).ravel()) / normD <= bound("drift_E_normD")
    np.testing.assert_allclose(eh, g["errHist"], rtol=bound("drift_errHist_rel"), atol=1e-15)
    for it in (1, 2):
        for key in ("A", "B", "C"):
            assert rel(tr[it][key], g[f"it{it}_{key}"]) <= bound("drift_it12_ABC")


@pytest.mark.parametrize("name", mc.names())
def test_golden_admission_rule(name):
    """Every tolerance a golden is held to is at least 100x its stored drift,
    and the perturbed reruns stopped at the same k."""
    g = mc.load(name)
    assert float(g["drift_k"]) == 0.0
    for q in mc.held(name):
        key, tol = mc.QUANTITIES[q]
        assert mc.MARGIN * float(g[key]) <= tol, (q, float(g[key]), tol)
    assert "L" in mc.held(name) and "errHist" in mc.held(name)
    assert ("O" in mc.held(name)) != ("O_normD" in mc.held(name))


@pytest.mark.parametrize("name", mc.names())
def test_unobserved_entries_stay_zero(name):
    g = mc.load(name)
    miss = ~g["observed"]
    assert miss.any()
    assert not g["O"][miss].any() and not g["E"][miss].any()


def test_stop_golden_stops_early():
    g = mc.load("m12x10x8_r2_stop")
    assert g["k"] == 9 < g["opts"]["maxIter"]


def test_tile_golden_has_a_whole_tile_missing():
    g = mc.load("m30_r3_tile")
    assert not g["observed"][:16, 0, :16].any()


@pytest.mark.parametrize("name", ["g12x10x8_r2", "g12x10x8_r2_stop", "qi12x10x8_r2", "g17x16x20_r8"])
def test_all_true_mask_is_the_reference_bitwise(name):
    from conftest import load_golden
    g = load_golden(name)
    ref = orc.triple_decomp_ADMM(g["D"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"])
    for observed in (None, np.ones(g["D"].shape, dtype=bool)):
        got = mo.triple_decomp_ADMM_masked(g["D"], observed, g["r"], g["opts"], g["A0"], g["B0"],
                                           g["C0"])
        assert got[6] == ref[6]
        for a, b in zip(got[:6], ref[:6]):
            np.testing.assert_array_equal(a, b)


def test_fill_values_never_enter():
    g = mc.load("m12x10x8_r2_stop")
    ref = mo.triple_decomp_ADMM_masked(g["D"], g["observed"], g["r"], g["opts"], g["A0"], g["B0"],
                                       g["C0"])
    for fill in (np.nan, 1e30):
        D = g["D"].copy(order="F")
        D[~g["observed"]] = fill
        got = mo.triple_decomp_ADMM_masked(D, g["observed"], g["r"], g["opts"], g["A0"], g["B0"],
                                           g["C0"])
        for a, b in zip(got[:6], ref[:6]):
            np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------
# argument errors that need no device
# ---------------------------------------------------------------------------
def test_observed_shape_mismatch_raises():
    import tritd
    g = mc.load("m12x10x8_r2")
    with pytest.raises(ValueError, match="observed must have the shape of D"):
        tritd.triple_decomp_ADMM(g["D"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                 observed=g["observed"][:, :, :-1])
    with pytest.raises(ValueError, match="observed must have the shape of D"):
        tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=12, n2=10, n3=8, D=g["D"],
                      observed=g["observed"].ravel())


def test_observed_with_float32_is_unsupported():
    import tritd
    from tritd import _lib
    g = mc.load("m12x10x8_r2")
    D32 = g["D"].astype(np.float32)
    with pytest.raises(tritd.TritdError) as e:
        tritd.triple_decomp_ADMM(D32, g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                 observed=g["observed"])
    assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED
    with pytest.raises(tritd.TritdError) as e:
        tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=12, n2=10, n3=8, D=D32,
                      observed=g["observed"], probe=False)
    assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED


def test_new_symbols_are_bound():
    from tritd import _lib
    for name in ("tritd_admm_masked_f64", "tritd_session_create_masked", "tritd_session_mask_info"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
