"""The C ABI of the session report (include/tritd.h; video_triple_comparison.m:56,
64-67) where no device is needed: the three symbols, the host
arithmetic of tritd.report_scores against tests/report_oracle.py (0/0 = NaN with
nothing missing included), and the first argument rule, reported before any HIP
call.  The rules past the NULL session need a session and cannot be reached
without a device; tests/test_gpu_report.py walks all of them, in their
documented order, on a live session.
"""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np

import report_oracle as ro
import tritd
from conftest import ROOT
from tritd import _lib, api, drivers

ARG = 1
NEW = ("tritd_session_report", "tritd_als_session_report", "tritd_session_report_ms")
lib = _lib.lib


def last_error():
    return lib.tritd_last_error().decode()


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def test_every_new_name_is_bound_and_exported():
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    assert set(NEW) <= set(re.findall(r"\bT (tritd_\w+)", out))
    header = open(os.path.join(ROOT, "include", "tritd.h")).read()
    assert "TRITD_REPORT_DEVICE = 1u" in header and _lib.REPORT_DEVICE == 1
    for name in NEW:  # each declaration cites the lines it replaces
        at = header.index(name + "(")
        assert "video_triple_comparison.m:56,64-67" in header[max(0, at - 4000):at], name
    assert hasattr(tritd, "report_scores") and "report_scores" in api.__all__
    assert hasattr(tritd.Session, "report") and hasattr(tritd.AlsSession, "report")
    assert hasattr(tritd.Session, "report_ms")
    assert inspect.signature(drivers.video_triple).parameters["session"].default is False
    sig = inspect.signature(tritd.Session.report).parameters
    assert list(sig)[1:] == ["X", "missing", "ssim", "x_device_ptr", "missing_device_ptr", "ldX", "ldM"]
    assert sig["ssim"].default is True and sig["ssim"].kind is inspect.Parameter.KEYWORD_ONLY


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_report_scores_equal_the_oracle():
    rng = np.random.default_rng(11)
    n1, n2, n3 = 13, 12, 5
    X = rng.uniform(0, 255, size=(n1, n2, n3))
    L = X + rng.normal(0, 3, size=X.shape)
    O = rng.normal(0, 1, size=X.shape) * (rng.random(X.shape) < 0.1)
    for m in (rng.random(X.shape) < 0.15, np.zeros(X.shape, dtype=bool), np.ones(X.shape, dtype=bool)):
        p = ro.parts(X, m, L, O)
        got = tritd.report_scores(p["sums"], p["frame_sq"], p["frame_ssim"], n1, n2)
        want = ro.figures_from_parts(p["sums"], p["frame_sq"], p["frame_ssim"], n1, n2)
        script = ro.driver_figures(X, m, L, O)
        for k in ro.FIGURES:
            assert same(got[k], want[k]), (k, got[k], want[k])
            assert same(got[k], script[k]) or abs(got[k] - script[k]) <= 1e-13 * abs(script[k]), k
        assert np.array_equal(got["psnr_frames"], want["psnr_frames"])
        assert np.array_equal(got["ssim_frames"], p["frame_ssim"])
    # nothing missing: rmse = 0 and nrmse = 0/0 = NaN, as MATLAB gives for an empty gt
    p = ro.parts(X, None, L, O)
    got = tritd.report_scores(p["sums"], p["frame_sq"], p["frame_ssim"], n1, n2)
    assert got["rmse"] == 0.0 and math.isnan(got["nrmse"]) and got["srmse"] > 0
    # everything missing: the observed pair is the empty one
    p = ro.parts(X, np.ones(X.shape, dtype=bool), L, O)
    got = tritd.report_scores(p["sums"], p["frame_sq"], p["frame_ssim"], n1, n2)
    assert got["srmse"] == 0.0 and math.isnan(got["snrmse"]) and got["rmse"] > 0
    # no SSIM asked for; a frame that L reproduces exactly has an infinite PSNR
    got = tritd.report_scores(p["sums"], np.array([0.0, 4.0]), None, n1, n2)
    assert math.isnan(got["ssim"]) and got["ssim_frames"] is None
    assert math.isinf(got["psnr_frames"][0]) and got["psnr_frames"][1] == ro.figures_from_parts(
        p["sums"], np.array([0.0, 4.0]), np.zeros(2), n1, n2)["psnr_frames"][1]
    # frames below the window: SSIM is -Inf and so is its mean
    got = tritd.report_scores(p["sums"], p["frame_sq"], np.full(n3, -np.inf), n1, n2)
    assert got["ssim"] == -math.inf


def test_shards_add_their_parts():
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 255, size=(20, 12, 4))
    L = X + rng.normal(0, 3, size=X.shape)
    O = rng.normal(0, 1, size=X.shape)
    m = rng.random(X.shape) < 0.15
    whole = ro.parts(X, m, L, O)
    halves = [ro.parts(X[a:b], m[a:b], L[a:b], O[a:b]) for a, b in ((0, 9), (9, 20))]
    sums = halves[0]["sums"] + halves[1]["sums"]
    fsq = halves[0]["frame_sq"] + halves[1]["frame_sq"]
    got = tritd.report_scores(sums, fsq, None, 20, 12)
    want = tritd.report_scores(whole["sums"], whole["frame_sq"], None, 20, 12)
    for k in ("rmse", "nrmse", "srmse", "snrmse", "trmse", "tnrmse", "psnr"):
        assert abs(got[k] - want[k]) <= 1e-13 * abs(want[k]), k


def test_null_session_is_the_first_rule_and_needs_no_device():
    X = np.zeros((4, 3, 2), order="F")
    sums, fsq = np.full(6, -7.0), np.full(2, -7.0)
    for fn in (lib.tritd_session_report, lib.tritd_als_session_report):
        # with every later rule broken too, the session is what is reported
        for args in ((ptr(X), 4, None, 0, ptr(sums), ptr(fsq), None, 0),
                     (None, 0, ptr(X), 0, None, None, None, 0)):
            assert fn(None, *args) == ARG
            assert "session is NULL" in last_error()
    ms = C.c_double(-1.0)
    assert lib.tritd_session_report_ms(None, C.byref(ms)) == ARG and "session is NULL" in last_error()
    assert (sums == -7.0).all() and (fsq == -7.0).all() and ms.value == -1.0
