"""Admission of the session-report cases (tests/report_cases.py)
on the CPU oracle alone: no case can let a GPU test pass vacuously.  For the
reference solver on the zero-filled data and for the masked solver, after
ITERS iterations:

  - the missing set is the driver's draw (exactly round(0.15 numel) entries)
    and it and its complement are non-empty in every frame;
  - all six sums are positive;
  - the SSIM frames are finite where min(n1, n2) >= 11 and -Inf below;
  - the figures from the raw parts are the figures the driver's own calls
    (evaluate, psnr_index, ssim_index) give;
  - the tolerances of tests/test_gpu_report.py stay near 1e-12: the ratios
    |L| / |L - X| on the missing entries and per frame, and |L + O| / |L + O - X|,
    stay below 5 (0.09 .. 2.5 on these cases).
"""
import numpy as np
import pytest

import report_cases as rc
import report_oracle as ro


def test_the_shapes_cover_the_layout_edges():
    shapes = {rc.case(n)["shape"] for n in rc.CASES}
    assert {(21, 7, 19), (16, 5, 16), (36, 21, 34), (70, 33, 5), (21, 13, 19)} == shapes
    assert {rc.case(n)["r"] for n in rc.CASES} == {2, 5, 11}
    assert rc.case(rc.QI_CASE)["opts"]["model"] == "qi" and rc.case(rc.QI_CASE)["r"] == 2
    assert sum(rc.STEPS) == rc.ITERS == 10


@pytest.mark.parametrize("name", rc.CASES)
def test_missing_is_the_drivers_draw(name):
    m, X = rc.missing(name), rc.case(name)["D"]
    assert m.dtype == np.bool_ and m.shape == X.shape and m.flags.f_contiguous
    assert int(m.sum()) == int(np.floor(rc.MISSING_RATIO * m.size + 0.5))
    assert m.any(axis=(0, 1)).all() and (~m).any(axis=(0, 1)).all()
    Y = rc.observed_data(name)
    assert (Y[m] == 0).all() and np.array_equal(Y[~m], X[~m])
    h = rc.holdout(name)
    assert (h & ~m).any() and (~h & ~m).any()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", rc.CASES)
def test_case_is_admitted_on_the_oracle(name, masked):
    c, m = rc.case(name), rc.missing(name)
    X = c["D"]
    n1, n2, _ = c["shape"]
    L, O = rc.oracle_run(name, masked)
    p = ro.parts(X, m, L, O)
    assert (p["sums"] > 0).all(), p["sums"]
    assert (p["frame_sq"] > 0).all()
    if min(n1, n2) >= 11:
        assert np.isfinite(p["frame_ssim"]).all()
        assert 0.01 < p["frame_ssim"].min() and p["frame_ssim"].max() < 0.6
    else:
        assert np.isneginf(p["frame_ssim"]).all()
    if masked:
        assert (O[m] == 0).all()  # a masked solve has O = 0 where unobserved
    # the parts and the host arithmetic give the driver's own figures
    want = ro.driver_figures(X, m, L, O)
    got = ro.figures_from_parts(p["sums"], p["frame_sq"], p["frame_ssim"], n1, n2)
    for k in ro.FIGURES:
        assert got[k] == pytest.approx(want[k], rel=1e-13) or (got[k] == want[k]), k
    assert np.allclose(got["psnr_frames"], want["psnr_frames"], rtol=1e-13, atol=0)
    # the tolerances the GPU tests will use
    ts, tf = ro.tolerances(X, m, L, O)
    assert ts.max() < 2e-12 and tf.max() < 2e-12
    nrm = lambda v: float(np.linalg.norm(np.asarray(v).ravel()))
    ratios = [nrm(L[m]) / nrm((L - X)[m]), nrm(L + O) / nrm(L + O - X)]
    ratios += [nrm(L[:, :, f]) / nrm(L[:, :, f] - X[:, :, f]) for f in range(X.shape[2])]
    assert 0.0 < min(ratios) and max(ratios) < 5.0, (min(ratios), max(ratios))


def test_nothing_missing_gives_nan_as_matlab_does():
    name = "full16_r5"
    c = rc.case(name)
    X = c["D"]
    L, O = rc.oracle_run(name, False)
    none = np.zeros(X.shape, dtype=bool)
    p = ro.parts(X, none, L, O)
    assert p["sums"][0] == 0.0 and p["sums"][1] == 0.0 and p["sums"][3] == p["sums"][5]
    got = ro.figures_from_parts(p["sums"], p["frame_sq"], p["frame_ssim"], *c["shape"][:2])
    want = ro.driver_figures(X, none, L, O)
    assert got["rmse"] == 0.0 == want["rmse"] and np.isnan(got["nrmse"]) and np.isnan(want["nrmse"])
    assert np.isneginf(got["ssim"]) and np.isneginf(want["ssim"])


def test_ssim_sensitivity_is_what_the_gpu_module_assumes():
    """the bound in tests/test_gpu_report.py's docstring (at most 1.2e-13 here)"""
    worst = 0.0
    for name in rc.CASES:
        if min(rc.case(name)["shape"][:2]) >= 11:
            for masked in (False, True):
                L, _ = rc.oracle_run(name, masked)
                worst = max(worst, ro.ssim_sensitivity(rc.case(name)["D"], L, np.random.default_rng(1)))
    assert 0.0 < worst <= 1.2e-13, worst
