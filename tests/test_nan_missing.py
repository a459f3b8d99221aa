"""NaN as missing (observed="nan", opts.nanmissing): what needs
no GPU.  The string is exactly "nan"; a float32 D is refused by the rule of
any mask; select_rank draws its holdout from ~isnan(X); the MEX gateway reads
opts.nanmissing after the required fields."""
import numpy as np
import pytest

import masked_als_cases as mac
import masked_cases as mc
import nan_missing_cases as nm

BAD = ["NaN", "nan ", "x"]


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    return t


@pytest.fixture(scope="module")
def gw(tmp_path_factory):
    return nm.build_gateway(tmp_path_factory)


@pytest.fixture(scope="module")
def g():
    g = mc.load("m12x10x8_r2")
    g["Dn"] = nm.with_nans(g["D"], g["observed"])
    return g


NCVX = dict(rho=1.0, lam=0.1, gamma_A=0.01, epsilon=1e-3, p=0.5, theta=1.0)


@pytest.mark.parametrize("bad", BAD)
def test_any_other_string_is_a_value_error_from_the_solvers(tritd, g, bad):
    f = (g["A0"], g["B0"], g["C0"])
    with pytest.raises(ValueError, match='the string "nan"'):
        tritd.triple_decomp_ADMM(g["Dn"], g["r"], g["opts"], *f, observed=bad)
    with pytest.raises(ValueError, match='the string "nan"'):
        tritd.triple_decomp_ALS(g["Dn"], g["r"], dict(maxIter=3, tol=0.0), *f, observed=bad)
    with pytest.raises(ValueError, match='the string "nan"'):
        tritd.triple_decomp_ncvx(g["Dn"], g["r"], *[NCVX[k] for k in NCVX], 3, 0.0, *f, observed=bad)


@pytest.mark.parametrize("bad", BAD)
def test_any_other_string_is_a_value_error_from_the_sessions(tritd, g, bad):
    f = (g["A0"], g["B0"], g["C0"])
    kw = dict(n1=12, n2=10, n3=8, observed=bad)
    o = dict(maxIter=3, tol=0.0)
    H = np.zeros(g["D"].shape, dtype=bool)
    H[0, 0, 0] = True
    with pytest.raises(ValueError, match='the string "nan"'):
        tritd.Session(g["r"], g["opts"], *f, D=g["Dn"], probe=False, **kw)
    with pytest.raises(ValueError, match='the string "nan"'):
        tritd.AlsSession(g["r"], o, *f, X=g["Dn"], **kw)
    with pytest.raises(ValueError, match='the string "nan"'):
        tritd.AlsSession(g["r"], o, *f, X=g["Dn"], ncvx=NCVX, **kw)
    with pytest.raises(ValueError, match='the string "nan"'):
        tritd.NcvxSession(g["r"], o, *f, X=g["Dn"], ncvx=NCVX, holdout=H, **kw)
    # beside a device-resident tensor too (the address is never used: the string is refused first)
    with pytest.raises(ValueError, match='the string "nan"'):
        tritd.AlsSession(g["r"], o, *f, x_device_ptr=4096, ldX=12, **kw)


def test_holdout_is_never_a_string(tritd, g):
    with pytest.raises(ValueError, match="holdout must be a logical array"):
        tritd.triple_decomp_ALS(g["Dn"], g["r"], dict(maxIter=3, tol=0.0), g["A0"], g["B0"], g["C0"],
                                observed="nan", holdout="nan")


def test_float32_with_nan_is_unsupported(tritd, g):
    from tritd import _lib
    with pytest.raises(tritd.TritdError) as e:
        tritd.triple_decomp_ADMM(nm.as_single(g["Dn"]), g["r"], g["opts"], g["A0"], g["B0"],
                                 g["C0"], observed="nan")
    assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED
    # a session: the library's own refusal, given before any device is touched
    with pytest.raises(tritd.TritdError) as e:
        tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=12, n2=10, n3=8,
                      D=nm.as_single(g["Dn"]), probe=False, observed="nan")
    assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED


def test_select_rank_draws_the_same_holdout(tritd, g):
    """H comes from ~isnan(X) on the host; the solver is handed "nan", not an array."""
    from tritd import drivers
    seen = []

    def stub(X, r, o, A0, B0, C0, *, device, return_iters, observed, holdout, patience):
        seen.append((observed, holdout))
        v = dict(valHist=np.array([1.0 / r]), best_iter=1, stop_reason=0, A_best=None, B_best=None,
                 C_best=None)
        return None, None, None, np.array([1.0]), 1, v

    a = drivers.select_rank(g["Dn"], "nan", (2, 3), holdout_ratio=0.2, seed=4, solver=stub)
    b = drivers.select_rank(g["Dn"], ~np.isnan(g["Dn"]), (2, 3), holdout_ratio=0.2, seed=4, solver=stub)
    assert np.array_equal(a["holdout"], b["holdout"]) and a["holdout"].any()
    assert not (a["holdout"] & np.isnan(g["Dn"])).any()
    assert a["rank"] == b["rank"] == 3
    assert [type(o) for o, _ in seen] == [str, str, np.ndarray, np.ndarray]
    assert seen[0][0] == "nan" and np.array_equal(seen[2][0], ~np.isnan(g["Dn"]))
    with pytest.raises(ValueError, match='the string "nan"'):
        drivers.select_rank(g["Dn"], "NaN", (2,), solver=stub)


def test_drivers_refuse_another_string(tritd, g):
    from tritd import drivers
    with pytest.raises(ValueError, match="use_mask must be"):
        drivers.traffic_triple(g["D"], r=2, use_mask="NaN", printer=lambda s: None)


# --- the MEX gateway (matlab/tritd_mex.cpp against tests/mock_mex) ------------
def test_gateway_missing_field_errors_are_unchanged(gw, g):
    o = g["opts"]
    names = ["mu", "rho", "lambda", "maxIter", "tol", "disp", "nanmissing"]  # no lambda2
    rc, err, _ = nm.gateway_admm(gw, g, g["Dn"], names, [float(o[n]) for n in names[:-1]] + [1.0])
    assert rc == 1
    assert err == "MATLAB:nonExistentField|Reference to non-existent field 'lambda2'."
    names = ["nanmissing", "rho", "lambda", "lambda2", "maxIter", "tol", "disp"]  # no mu, the first read
    rc, err, _ = nm.gateway_admm(gw, g, g["Dn"], names, [1.0] + [float(o[n]) for n in names[1:]])
    assert rc == 1
    assert err == "MATLAB:nonExistentField|Reference to non-existent field 'mu'."
    ga = mac.load("oals12x10x8_r2")
    rc, err, _ = nm.gateway_als(gw, ga, ga["X"], ["nanmissing", "tol"], [1.0, 1e-5])
    assert rc == 1
    assert err == "MATLAB:nonExistentField|Reference to non-existent field 'maxIter'."
    rc, err, _ = nm.gateway_als(gw, ga, ga["X"], ["maxIter", "nanmissing"], [5.0, 1.0])
    assert err == "MATLAB:nonExistentField|Reference to non-existent field 'tol'."


def test_gateway_without_a_gpu_fails_in_the_solver_not_in_the_parse(tritd, gw, g):
    if tritd.device_count() > 0:
        pytest.skip("GPU visible")
    o = g["opts"]
    names = nm.ADMM_FIELDS + ["nanmissing"]
    rc, err, _ = nm.gateway_admm(gw, g, g["Dn"], names, [float(o[n]) for n in nm.ADMM_FIELDS] + [1.0])
    assert rc == 1 and err.startswith("tritd:solver|") and "no HIP device" in err
    ga = mac.load("oals12x10x8_r2")
    Xn = nm.with_nans(ga["X"], ga["observed"])
    rc, err, _ = nm.gateway_als(gw, ga, Xn, ["maxIter", "tol", "nanmissing"],
                                [float(ga["opts"]["maxIter"]), float(ga["opts"]["tol"]), 1.0])
    assert rc == 1 and err.startswith("tritd:solver|") and "no HIP device" in err


def test_gateway_single_with_nanmissing_is_the_librarys_refusal(gw, g):
    o = g["opts"]
    names = nm.ADMM_FIELDS + ["nanmissing"]
    vals = [float(o[n]) for n in nm.ADMM_FIELDS]
    rc, err, _ = nm.gateway_admm(gw, g, g["Dn"], names, vals + [1.0], single=True)
    assert rc == 1 and err.startswith("tritd:solver|libtritd: ")
    assert "double D only" in err and "(status 7)" in err
