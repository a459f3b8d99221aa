"""The video driver's report from a session on the GPU (DESIGN.md §17;
video_triple_comparison.m:56,64-67): the six masked sums, the frame squares and
the SSIM frames, taken from the session's resident tensors without L or O ever
being downloaded.  Inputs: tests/report_cases.py, admitted on the CPU by
tests/test_report_cases.py.

Every comparison tests the kernel, not the iterates: the reference is
tests/report_oracle.py applied to the session's own get() factors and O, with L
from the oracle's triple_product.  Tolerances come from the reference alone
(report_oracle.tolerances, after boundary_cases.rre_reference): the
denominators and S2 take RTOL_SUM = 1e-12; S0, S4 and frame_sq take
RTOL_SUM + 2 TOL_TP |L or L+O| / |difference| over the same index set,
TOL_TP = 1e-13 (they stay below 2e-12 on these cases).  SSIM per frame takes
the existing primitive's 1e-11 (tests/test_gpu_metrics.py) plus ten times the
largest relative change of the oracle's ssim_index when L is perturbed
elementwise by +-TOL_TP: measured on the CPU for these cases after 10
iterations (tests/test_report_cases.py keeps it there), that change is at most
1.11e-13 (sweep36_r11, masked), so SSIM_RTOL = 1e-11 + 10 x 1.11e-13.

1. Sums, frame_sq and SSIM against the oracle after 0, 3 and 3 + 7 iterations,
   for a session on the zero-filled data, a masked one (O = 0 at unobserved
   entries) and a holdout one, every case; and after 3 iterations at one rank
   per padded rank 16 ... 256 (the cases of tests/sweep_cases.py).
2. X and missing inside the three buffer forms of boundary_cases.padded with
   NaN / 0xFF fill: no NaN in any output; the host and TRITD_REPORT_DEVICE
   forms give the same bits; two calls give the same bits.
3. A twin session that never called report returns bitwise the same get()
   after further iterations.
4. A sub-range [5, n1 - 4) without a communicator gives the standalone
   problem's parts, with X inside the whole tensor (ldX = n1); SSIM there is
   TRITD_ERR_ARG.
5. A plain AlsSession (O = 0), a nonconvex one (the O of get_O) and one stopped
   by tol (the O of k - 1).
6. An fp32 session is TRITD_ERR_UNSUPPORTED.
7. drivers.video_triple(session=True) prints the reference's line with the
   oracle's figures on the A, B, C, O it returns; missing_ratio = 0 gives
   rmse 0 and nrmse NaN, as in MATLAB.
8. Every argument rule, in the documented order, on a live session.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import boundary_cases as bc
import report_cases as rc
import report_oracle as ro
import sweep_cases as sc
import tritd_oracle as orc
from conftest import load_golden

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED = 1, 7
SSIM_RTOL = 1e-11 + 10 * 1.11e-13
FORMS = ("plain", "masked", "holdout")
RUNS = [(n, f) for n in rc.CASES for f in FORMS if not (n == rc.QI_CASE and f == "holdout")]


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def hip(tritd):
    from tritd import hip as h
    return h


def open_session(tritd, name, form, **kw):
    c = rc.case(name)
    n1, n2, n3 = c["shape"]
    if form in ("masked", "holdout"):
        kw["observed"] = ~rc.missing(name)
    if form == "holdout":
        kw["holdout"] = rc.holdout(name)
    return tritd.Session(c["r"], c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                         D=rc.observed_data(name), probe=False, device=0, **kw)


def check_parts(rep, X, missing, L, O, what=""):
    """sums, frame_sq, SSIM frames and the eight figures against the oracle's"""
    want = ro.parts(X, missing, L, O)
    ts, tf = ro.tolerances(X, missing, L, O)
    print(what, "sums rel", np.abs(rep["sums"] - want["sums"]) / np.maximum(want["sums"], 1e-300), "tol", ts)
    for q in range(6):
        assert rep["sums"][q] == pytest.approx(want["sums"][q], rel=ts[q], abs=0), (what, q)
    rel = np.abs(rep["frame_sq"] - want["frame_sq"]) / want["frame_sq"]
    print(what, "frame_sq rel", rel.max(), "tol", tf.max())
    assert (rel <= tf).all(), (what, rel.max())
    if rep["ssim_frames"] is not None:
        fin = np.isfinite(want["frame_ssim"])
        assert fin.all() == (min(X.shape[:2]) >= 11) and (fin.all() or not fin.any())
        if fin.all():
            srel = np.abs(rep["ssim_frames"] - want["frame_ssim"]) / np.abs(want["frame_ssim"])
            print(what, "ssim rel", srel.max())
            assert (srel <= SSIM_RTOL).all(), (what, srel.max())
        else:
            assert np.isneginf(rep["ssim_frames"]).all()
    fig = ro.figures_from_parts(rep["sums"], rep["frame_sq"],
                                rep["ssim_frames"] if rep["ssim_frames"] is not None else np.zeros(X.shape[2]),
                                *X.shape[:2])
    for k in ro.FIGURES[:7]:  # the host arithmetic is the oracle's
        assert rep[k] == fig[k] or (math.isnan(rep[k]) and math.isnan(fig[k])), k
    return want


# --- 1. / 3. sums against the oracle, twin sessions ---------------------------------------
@functools.lru_cache(maxsize=None)
def session_run(name, form):
    """One session that reports before the first iteration, after 3 and after
    3 + 7, and a twin that never does: -> dict(rep0, rep3, rep10, again10, get0,
    get3, get10, twin3, twin10).  Computed once per (case, form) and shared."""
    import tritd
    s, t = open_session(tritd, name, form), open_session(tritd, name, form)
    X, m = rc.case(name)["D"], rc.missing(name)
    try:
        out = dict(get0=s.get(), rep0=s.report(X, m))
        for s_, keys in ((s, ("rep", "get")), (t, (None, "twin"))):
            for iters, tag in zip(rc.STEPS, ("3", "10")):
                s_.run(iters)
                if keys[0]:
                    out[keys[0] + tag] = s_.report(X, m)
                out[keys[1] + tag] = s_.get()
        out["again10"] = s.report(X, m)
    finally:
        s.close()
        t.close()
    return out


@pytest.mark.parametrize("name,form", RUNS)
def test_parts_equal_the_oracle_on_the_sessions_own_iterates(tritd, name, form):
    r = session_run(name, form)
    c, m = rc.case(name), rc.missing(name)
    X = c["D"]
    for tag in ("0", "3", "10"):
        g = r["get" + tag]
        assert g["k"] == int(tag)
        L = orc.triple_product(g["A"], g["B"], g["C"], model=c["model"])
        O = g["O"] if g["k"] else np.zeros(X.shape, order="F")
        if form != "plain" and g["k"]:
            assert (O[m] == 0).all() and (O != 0).any()
        want = check_parts(r["rep" + tag], X, m, L, O, "%s/%s/%s" % (name, form, tag))
        assert (want["sums"] > 0).all()
    # before the first iteration O = 0: S2 = S3, and S4 is the sum of the frame squares
    assert r["rep0"]["sums"][2] == r["rep0"]["sums"][3]
    assert r["rep0"]["sums"][4] == pytest.approx(r["rep0"]["frame_sq"].sum(), rel=1e-12)
    # two calls give the same bits
    for k in ("sums", "frame_sq", "ssim_frames"):
        assert r["again10"][k].tobytes() == r["rep10"][k].tobytes(), k


@pytest.mark.parametrize("name,form", RUNS)
def test_report_leaves_the_iterates_untouched(tritd, name, form):
    r = session_run(name, form)
    for tag in ("3", "10"):
        a, b = r["get" + tag], r["twin" + tag]
        assert a["k"] == b["k"]
        for key in ("A", "B", "C", "O", "E", "errHist"):
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape
            assert a[key].tobytes(order="A") == b[key].tobytes(order="A"), (tag, key)


@pytest.mark.parametrize("r", bc.RANKS)
def test_every_padded_rank(tritd, r):
    """one rank per padded rank 16, 32, 48, 64, 128, 256 (sweep_cases.e_active_case):
    the slice staging has a form of its own at each, and 256 is the one that spills"""
    c = sc.e_active_case(r)
    X = c["D"]
    n1, n2, n3 = X.shape
    m = np.asfortranarray(np.random.default_rng(r).random(X.shape) < rc.MISSING_RATIO)
    s = tritd.Session(r, c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3, D=X, probe=False,
                      device=0)
    try:
        s.run(3)
        g = s.get()
        want = check_parts(s.report(X, m), X, m, orc.triple_product(g["A"], g["B"], g["C"]), g["O"],
                           "rank %d" % r)
        assert (want["sums"] > 0).all() and np.isfinite(want["frame_ssim"]).all()
    finally:
        s.close()


# --- 2. leading dimensions --------------------------------------------------------------
@pytest.mark.parametrize("name", ["pad21_r5", "sweep36_r5"])
def test_padding_is_never_read_and_the_device_form_gives_the_same_bits(tritd, hip, name):
    c, m = rc.case(name), rc.missing(name)
    X = c["D"]
    n1 = X.shape[0]
    s = open_session(tritd, name, "masked")
    try:
        s.run(4)
        base = s.report(X, m)
        for form in bc.FORMS:
            Xb, ldX, off = bc.padded(X, form)                       # NaN outside the rows
            Mb, ldM, offm = bc.padded(m.view(np.uint8), form, fill=0xFF)
            assert ldX == ldM and off == offm and (form == "contig" or np.isnan(Xb).any())
            host = s.report(Xb[off:off + n1], Mb[off:off + n1].view(np.bool_))
            dX, dM = hip.DeviceArray.from_host(Xb), hip.DeviceArray.from_host(Mb)
            try:
                dev = s.report(x_device_ptr=dX.ptr + 8 * off, missing_device_ptr=dM.ptr + off,
                               ldX=ldX, ldM=ldM)
                dev2 = s.report(x_device_ptr=dX.ptr + 8 * off, missing_device_ptr=dM.ptr + off,
                                ldX=ldX, ldM=ldM)
            finally:
                dX.free()
                dM.free()
            for res in (host, dev, dev2):
                for k in ("sums", "frame_sq", "ssim_frames", "psnr_frames"):
                    assert not np.isnan(res[k]).any(), (form, k)   # a NaN: padding was read
                    assert res[k].tobytes() == base[k].tobytes(), (form, k)
    finally:
        s.close()


def test_no_mask_no_ssim_and_the_kernel_time(tritd):
    name = "sweep36_r5"
    c = rc.case(name)
    X = c["D"]
    s = open_session(tritd, name, "plain")
    try:
        s.run(5)
        g = s.get()
        L = orc.triple_product(g["A"], g["B"], g["C"])
        rep = s.report(X, ssim=False)  # nothing missing: the first pair is the empty one
        assert rep["ssim_frames"] is None and math.isnan(rep["ssim"])
        check_parts(rep, X, None, L, g["O"], "no mask")
        assert rep["sums"][0] == 0.0 and rep["sums"][1] == 0.0 and rep["sums"][3] == rep["sums"][5]
        assert rep["rmse"] == 0.0 and math.isnan(rep["nrmse"])
        assert s.report_ms() == 0.0
        s.set_timing(True)
        full = s.report(X, rc.missing(name))
        assert 0.0 < s.report_ms() < 1e3
        assert full["frame_sq"].tobytes() == rep["frame_sq"].tobytes()
    finally:
        s.close()


# --- 4. a sub-range of the rows -----------------------------------------------------------
def test_sub_range_gives_the_standalone_parts_and_refuses_ssim(tritd):
    name = "sweep36_r5"
    c, m = rc.case(name), rc.missing(name)
    X, Y = c["D"], rc.observed_data(name)
    n1, n2, n3 = c["shape"]
    i0, i1 = bc.sub_range(n1)
    assert (i0, i1) == (5, n1 - 4)
    Ys = np.asfortranarray(Y[i0:i1])
    alone = tritd.Session(c["r"], c["opts"], np.asfortranarray(c["A0"][i0:i1]), c["B0"], c["C0"],
                          n1=i1 - i0, n2=n2, n3=n3, D=Ys, probe=False, device=0)
    shard = tritd.Session(c["r"], c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                          i0=i0, i1=i1, D=Ys, probe=False, device=0)
    try:
        alone.run(rc.ITERS)
        shard.run(rc.ITERS)
        want = alone.report(np.asfortranarray(X[i0:i1]), np.asfortranarray(m[i0:i1]), ssim=False)
        g = alone.get()
        check_parts(want, X[i0:i1], m[i0:i1], orc.triple_product(g["A"], g["B"], g["C"]), g["O"], "alone")
        # X and the mask inside the whole tensors: their strides give ldX = ldM = n1
        got = shard.report(X[i0:i1], m[i0:i1], ssim=False)
        for k in ("sums", "frame_sq"):
            assert got[k].tobytes() == want[k].tobytes(), k
        # the shard's psnr is over whole frames of n1 rows: a caller adds frame_sq first
        assert np.array_equal(got["psnr_frames"], tritd.report_scores(
            want["sums"], want["frame_sq"], None, n1, n2)["psnr_frames"])
        with pytest.raises(tritd.TritdError) as e:
            shard.report(X[i0:i1], m[i0:i1])
        assert e.value.status == ARG and "all rows" in str(e.value)
        again = shard.report(X[i0:i1], m[i0:i1], ssim=False)  # and the session still works
        assert again["sums"].tobytes() == want["sums"].tobytes()
    finally:
        alone.close()
        shard.close()


# --- 5. ALS sessions -----------------------------------------------------------------------
def test_plain_als_session_has_no_outlier_term(tritd):
    name = "pad21_r5"
    c, m = rc.case(name), rc.missing(name)
    X = c["D"]
    n1, n2, n3 = c["shape"]
    s = tritd.AlsSession(c["r"], sc.ALS_OPTS, c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                         X=rc.observed_data(name), device=0, observed=~m)
    try:
        for iters in (0, 3):
            s.run(iters)
            g = s.get()
            rep = s.report(X, m)
            check_parts(rep, X, m, orc.triple_product(g["A"], g["B"], g["C"]), np.zeros(X.shape),
                        "als %d" % iters)
            assert rep["sums"][2] == rep["sums"][3]
    finally:
        s.close()


def ncvx_session(tritd, X, r, A0, B0, C0, prm):
    n1, n2, n3 = X.shape
    return tritd.AlsSession(r, dict(maxIter=prm["maxIter"], tol=prm["tol"]), A0, B0, C0, n1=n1, n2=n2,
                            n3=n3, X=X, device=0,
                            ncvx={k: prm[k] for k in ("rho", "lam", "gamma_A", "epsilon", "p", "theta")})


def test_ncvx_session_uses_the_O_of_get_O(tritd):
    name = "sweep36_r5"
    c, m = rc.case(name), rc.missing(name)
    X = c["D"]
    s = ncvx_session(tritd, rc.observed_data(name), c["r"], c["A0"], c["B0"], c["C0"], sc.NCVX_PARAMS)
    try:
        for iters in (0, 3, sc.NCVX_PARAMS["maxIter"]):
            s.run(iters)
            g, O = s.get(), s.get_O()
            assert (O != 0).any() == (g["k"] > 0)
            check_parts(s.report(X, m), X, m, orc.triple_product(g["A"], g["B"], g["C"]), O,
                        "ncvx %d" % g["k"])
        assert s.sync() == (sc.NCVX_PARAMS["maxIter"], False)
    finally:
        s.close()


def test_ncvx_session_stopped_by_tol_uses_the_previous_O(tritd):
    g = load_golden("nc20x24x18_r3_stop")
    o = g["opts"]
    X = np.asfortranarray(g["X"])
    m = np.asfortranarray(np.random.default_rng(6).random(X.shape) < 0.15)
    s = ncvx_session(tritd, X, g["r"], g["A0"], g["B0"], g["C0"], dict(o, lam=o["lambda"]))
    try:
        s.run(o["maxIter"])
        assert s.sync() == (g["k"], True)
        f, O = s.get(), s.get_O()
        L = orc.triple_product(f["A"], f["B"], f["C"])
        rep = s.report(X, m)
        # X is the data the session fitted: L + O is close to it, and the tolerance follows
        check_parts(rep, X, m, L, O, "ncvx stop")
    finally:
        s.close()


# --- 6. fp32 ---------------------------------------------------------------------------------
def test_fp32_session_is_unsupported(tritd):
    c = rc.case("full16_r5")
    n1, n2, n3 = c["shape"]
    s = tritd.Session(c["r"], c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                      D=np.asfortranarray(c["D"], dtype=np.float32), probe=False, device=0)
    try:
        s.run(2)
        with pytest.raises(tritd.TritdError) as e:
            s.report(c["D"], ssim=False)
        assert e.value.status == UNSUPPORTED and "fp64 sessions only" in str(e.value)
        assert s.get()["k"] == 2
    finally:
        s.close()


# --- 7. the video driver ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sweep36_r5", "pad21_r5"])
def test_video_driver_session_path_prints_the_line(tritd, name):
    from tritd import drivers
    c = rc.case(name)
    X = c["D"]
    lines = []
    out = drivers.video_triple(X, r=c["r"], missing_ratio=0.15, opts=dict(c["opts"], disp=0),
                               A0=c["A0"], B0=c["B0"], C0=c["C0"], printer=lines.append, session=True)
    assert len(lines) == 2 and lines[0] == "\n===== Dataset: data Missing Radio 0.150====="
    m = out["mask"]
    assert int(m.sum()) == int(np.floor(0.15 * m.size + 0.5))
    L = orc.triple_product(out["A"], out["B"], out["C"])
    want = ro.driver_figures(X, m, L, out["O"])
    ts, tf = ro.tolerances(X, m, L, out["O"])
    # a figure is the square root (or a ratio of two roots) of sums within ts; a frame's
    # PSNR is 10 log10 of a quotient within tf, so it moves by 10 / ln(10) of that
    for k in ro.FIGURES[:6]:
        assert out[k] == pytest.approx(want[k], rel=ts.max(), abs=0), k
    assert out["psnr"] == pytest.approx(want["psnr"], rel=1e-13, abs=10.0 / math.log(10.0) * tf.max())
    if min(X.shape[:2]) >= 11:
        assert out["ssim"] == pytest.approx(want["ssim"], rel=SSIM_RTOL, abs=0)
    else:
        assert out["ssim"] == -math.inf == want["ssim"]
    assert lines[1] == drivers._VIDEO_LINE % (tuple(out[k] for k in ro.FIGURES) + (out["time"],))
    assert lines[1].startswith("TRIPLE ADMM - RMSE: %.4e, NRMSE: %.4e, SRMSE:" % (out["rmse"], out["nrmse"]))
    assert np.array_equal(out["X_hat"], tritd.triple_product(out["A"], out["B"], out["C"]))


def test_video_driver_session_path_with_nothing_missing_and_groundtruth(tritd):
    import foreground_cases as fc
    import foreground_oracle as fo
    from tritd import drivers
    c = fc.case("pad21_r5")
    lines = []
    out = drivers.video_triple(c["D"], r=c["r"], missing_ratio=0, opts=dict(c["opts"], disp=0),
                               A0=c["A0"], B0=c["B0"], C0=c["C0"], printer=lines.append, session=True,
                               groundtruth=c["G"])
    assert out["rmse"] == 0.0 and math.isnan(out["nrmse"])  # norm([]) = 0, 0/0 = NaN, as in MATLAB
    assert "RMSE: 0.0000e+00, NRMSE: nan," in lines[1]
    assert out["srmse"] > 0 and out["snrmse"] > 0
    counts = fo.eval_counts(out["O"], c["G"], 50.0)
    assert len(lines) == 7 and lines[2:] == fo.report_lines(fo.scores(counts, out["O"].size))
    assert (out["fg_counts"] == counts).all() and (out["fg_mask"] == fo.pred_mask(out["O"], 50.0)).all()
    # the one-shot path prints the same figures for the same start
    ref = []
    one = drivers.video_triple(c["D"], r=c["r"], missing_ratio=0, opts=dict(c["opts"], disp=0),
                               A0=c["A0"], B0=c["B0"], C0=c["C0"], printer=ref.append, groundtruth=c["G"])
    assert ref[2:] == lines[2:]
    for k in ("srmse", "snrmse", "trmse", "tnrmse", "psnr"):
        assert out[k] == pytest.approx(one[k], rel=1e-9), k


# --- 8. the argument rules --------------------------------------------------------------------
def test_argument_rules_in_their_order_on_a_live_session(tritd):
    from tritd import _lib
    name = "pad21_r5"
    c, m = rc.case(name), rc.missing(name)
    X = c["D"]
    nl, n2, n3 = X.shape
    mb = np.asfortranarray(m.view(np.uint8))
    s = open_session(tritd, name, "plain")
    als = tritd.AlsSession(c["r"], sc.ALS_OPTS, c["A0"], c["B0"], c["C0"], n1=nl, n2=n2, n3=n3,
                           X=rc.observed_data(name), device=0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    sums, fsq, fss = np.full(6, -7.0), np.full(n3, -7.0), np.full(n3, -7.0)
    # each entry breaks one rule more than the next: the first broken one is reported
    rules = [((None, nl - 1, p(mb), nl - 1, None, None, p(fss), 0), "X is NULL"),
             ((p(X), nl - 1, p(mb), nl - 1, None, None, p(fss), 0), "ldX smaller than the shard"),
             ((p(X), nl, p(mb), nl - 1, None, None, p(fss), 0), "ldM smaller than the shard"),
             ((p(X), nl, p(mb), nl, None, None, p(fss), 0), "both NULL")]
    try:
        s.run(2)
        for handle, fn in ((s._s, _lib.lib.tritd_session_report), (als._s, _lib.lib.tritd_als_session_report)):
            for args, msg in rules:
                assert fn(handle, *args) == ARG, args
                assert msg in _lib.lib.tritd_last_error().decode(), (args, msg)
            # a NULL mask's leading dimension is not looked at; one output is enough
            _lib.check(fn(handle, p(X), nl, None, 0, p(sums), None, None, 0))
            _lib.check(fn(handle, p(X), nl, None, 0, None, p(fsq), None, 0))
            assert (sums != -7.0).all() and (fsq != -7.0).all() and (fss == -7.0).all()
            sums[:], fsq[:] = -7.0, -7.0
        assert _lib.lib.tritd_session_report_ms(s._s, None) == ARG
        assert "kernel_ms is NULL" in _lib.lib.tritd_last_error().decode()
    finally:
        s.close()
        als.close()
