"""The C ABI of the foreground detection (include/tritd.h, eval of
video_triple_comparison.m:316-371) where no device is needed: the symbols, the
host arithmetic of tritd_foreground_scores against tests/foreground_oracle.py,
and the argument rules, each reported before the first HIP call and in the
documented order (NULL session or F, dimensions, thr, both outputs NULL,
leading dimensions).  Without a visible GPU an otherwise valid primitive call
ends at TRITD_ERR_NODEV; with one it runs.  The session forms' rules past the
NULL session need a session: tests/test_gpu_foreground.py.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import foreground_oracle as fo
import tritd
from conftest import ROOT
from tritd import _lib, api, drivers

ARG, NODEV = 1, 6
NEW = ("tritd_session_foreground", "tritd_session_foreground_ms", "tritd_als_session_foreground", "tritd_foreground_f64",
       "tritd_foreground_f32", "tritd_dev_foreground_f64", "tritd_dev_foreground_f32",
       "tritd_foreground_scores")
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
    exported = set(re.findall(r"\bT (tritd_\w+)", out))
    assert set(NEW) <= exported
    header = open(os.path.join(ROOT, "include", "tritd.h")).read()
    assert "TRITD_FG_DEVICE = 1u" in header and _lib.FG_DEVICE == 1
    for name in NEW:  # each declaration cites the lines it restates
        at = header.index(name + "(")
        assert "video_triple_comparison.m:316-371" in header[max(0, at - 2500):at], name
    for name in ("foreground_eval", "foreground_scores"):
        assert hasattr(tritd, name) and name in api.__all__
    assert hasattr(tritd.Session, "foreground") and hasattr(tritd.AlsSession, "foreground")


def c_scores(counts, numel):
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1, 4)
    total = np.zeros(4, dtype=np.int64)
    v = [C.c_double(-1.0) for _ in range(4)]
    st = lib.tritd_foreground_scores(ptr(counts), counts.shape[0], numel, ptr(total),
                                     *(C.byref(x) for x in v))
    assert st == 0, last_error()
    return dict(total=total, precision=v[0].value, recall=v[1].value, f1=v[2].value, pwc=v[3].value)


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_scores_equal_the_oracle():
    rng = np.random.default_rng(5)
    sets = [rng.integers(0, 2 ** 40, size=(7, 4)), rng.integers(0, 50, size=(1, 4)),
            np.zeros((3, 4), dtype=np.int64), np.array([[0, 5, 0, 3]]), np.array([[0, 0, 4, 3]]),
            np.zeros((0, 4), dtype=np.int64)]
    for counts in sets:
        for numel in (0, 1, 12345, 2 ** 45):
            got, want = c_scores(counts, numel), fo.scores(counts, numel)
            assert (got["total"] == want["total"]).all()
            for k in ("precision", "recall", "f1", "pwc"):
                assert same(got[k], want[k]), (k, got[k], want[k], counts, numel)
            py = tritd.foreground_scores(counts, numel)
            assert (py["total"] == want["total"]).all()
            assert all(same(py[k], want[k]) for k in ("precision", "recall", "f1", "pwc"))
    z = c_scores(np.zeros((2, 4)), 8)
    assert math.isnan(z["precision"]) and math.isnan(z["recall"]) and math.isnan(z["f1"])
    assert z["pwc"] == 0.0


def test_scores_outputs_are_optional_and_sizes_checked():
    counts = np.array([[3, 1, 2, 10]], dtype=np.int64)
    assert lib.tritd_foreground_scores(ptr(counts), 1, 16, None, None, None, None, None) == 0
    f1 = C.c_double(0)
    assert lib.tritd_foreground_scores(ptr(counts), 1, 16, None, None, None, C.byref(f1), None) == 0
    assert f1.value == fo.scores(counts, 16)["f1"]
    assert lib.tritd_foreground_scores(None, 1, 16, None, None, None, None, None) == ARG
    assert "counts is NULL" in last_error()
    assert lib.tritd_foreground_scores(ptr(counts), -1, 16, None, None, None, None, None) == ARG
    assert lib.tritd_foreground_scores(ptr(counts), 1, -1, None, None, None, None, None) == ARG
    assert "sizes must be >= 0" in last_error()


N1, N2, NF = 6, 5, 3


@pytest.fixture(scope="module")
def bufs():
    rng = np.random.default_rng(3)
    F = np.asfortranarray(rng.normal(0, 60, size=(N1, N2, NF)))
    return dict(F=F, F32=np.asfortranarray(F, dtype=np.float32),
                G=np.asfortranarray(rng.choice(np.array([0, 170, 255], dtype=np.uint8), size=F.shape)),
                P=np.full(F.shape, 0xAB, dtype=np.uint8, order="F"),
                counts=np.full((NF, 4), -7, dtype=np.int64))


def host_call(b, f32=False, **kw):
    a = dict(F=ptr(b["F32"] if f32 else b["F"]), gt=ptr(b["G"]), n1=N1, n2=N2, nf=NF, thr=50.0,
             pred=ptr(b["P"]), counts=ptr(b["counts"]))
    a.update(kw)
    fn = lib.tritd_foreground_f32 if f32 else lib.tritd_foreground_f64
    return fn(a["F"], a["gt"], a["n1"], a["n2"], a["nf"], a["thr"], a["pred"], a["counts"])


def dev_call(b, f32=False, **kw):
    """the device form on HOST addresses: only calls that the rules refuse"""
    a = dict(F=ptr(b["F32"] if f32 else b["F"]), ldF=N1, gt=ptr(b["G"]), ldG=N1, n1=N1, n2=N2, nf=NF,
             thr=50.0, pred=ptr(b["P"]), ldP=N1, counts=ptr(b["counts"]))
    a.update(kw)
    fn = lib.tritd_dev_foreground_f32 if f32 else lib.tritd_dev_foreground_f64
    return fn(a["F"], a["ldF"], a["gt"], a["ldG"], a["n1"], a["n2"], a["nf"], a["thr"], a["pred"],
              a["ldP"], a["counts"], None)


RULES = [  # (changes, message), in the order the rules are reported
    (dict(F=None), "F is NULL"),
    (dict(n1=0), "sizes must be positive"),
    (dict(n2=-1), "sizes must be positive"),
    (dict(nf=0), "sizes must be positive"),
    (dict(thr=-1e-300), "thr must be >= 0"),
    (dict(thr=float("nan")), "thr must be >= 0"),
    (dict(thr=-float("inf")), "thr must be >= 0"),
    (dict(gt=None, pred=None), "gt and pred are both NULL"),
    (dict(counts=None), "counts is NULL"),
]
LD_RULES = [(dict(ldF=N1 - 1), "ldF smaller than n1"), (dict(ldG=N1 - 1), "ldG smaller than n1"),
            (dict(ldP=N1 - 1), "ldP smaller than n1")]


@pytest.mark.parametrize("f32", [False, True])
def test_each_argument_rule_is_reported(bufs, f32):
    for changes, msg in RULES:
        for call in (host_call, dev_call):
            assert call(bufs, f32, **changes) == ARG, (call.__name__, changes)
            assert msg in last_error(), (call.__name__, changes, last_error())
    for changes, msg in LD_RULES:
        assert dev_call(bufs, f32, **changes) == ARG, changes
        assert msg in last_error()
    # refused calls write nothing
    assert (bufs["P"] == 0xAB).all() and (bufs["counts"] == -7).all()


def test_rules_are_reported_in_the_documented_order(bufs):
    order = [dict(F=None), dict(n1=0), dict(thr=-1.0), dict(gt=None, pred=None), dict(ldG=N1 - 1)]
    msgs = ["F is NULL", "sizes must be positive", "thr must be >= 0", "both NULL", "ldG smaller"]
    for x in range(len(order)):
        for y in range(x + 1, len(order)):
            both = dict(order[y], **order[x])
            assert dev_call(bufs, **both) == ARG
            assert msgs[x] in last_error(), (order[x], order[y], last_error())


def test_null_session_is_an_argument_error(bufs):
    for fn in (lib.tritd_session_foreground, lib.tritd_als_session_foreground):
        assert fn(None, 50.0, ptr(bufs["G"]), N1, ptr(bufs["P"]), N1, ptr(bufs["counts"]), 0) == ARG
        assert "session is NULL" in last_error()


def test_a_valid_primitive_call_needs_a_device(bufs):
    """no CPU fallback: TRITD_ERR_NODEV without a GPU, the oracle's result with one"""
    gpu = tritd.device_count() > 0
    for f32 in (False, True):
        b = dict(bufs, P=bufs["P"].copy(order="F"), counts=bufs["counts"].copy())
        st = host_call(b, f32)
        if not gpu:
            assert st == NODEV, last_error()
            assert (b["P"] == 0xAB).all() and (b["counts"] == -7).all()
            with pytest.raises(tritd.TritdError) as e:
                tritd.foreground_eval(b["F32"] if f32 else b["F"], b["G"])
            assert e.value.status == NODEV
        else:
            assert st == 0, last_error()
            F = b["F32"] if f32 else b["F"]
            assert (b["P"].view(np.bool_) == fo.pred_mask(F, 50.0)).all()
            assert (b["counts"] == fo.eval_counts(F, b["G"], 50.0)).all()


def test_python_forms_check_shapes_before_any_c_call(bufs):
    with pytest.raises(ValueError):
        tritd.foreground_eval(bufs["F"], bufs["G"][:, :, :2])


class Spy:
    """``drivers.api`` with every attribute access recorded"""

    def __init__(self, real):
        self._real, self.used = real, []

    def __getattr__(self, name):
        self.used.append(name)
        return getattr(self._real, name)


def test_video_triple_without_groundtruth_does_not_touch_the_new_path(monkeypatch):
    spy = Spy(drivers.api)
    monkeypatch.setattr(drivers, "api", spy)
    X = np.asfortranarray(np.random.default_rng(1).uniform(0, 255, size=(12, 11, 4)))
    lines = []
    try:
        out = drivers.video_triple(X, r=2, opts=dict(drivers.VIDEO_OPTS, maxIter=2, disp=0),
                                   printer=lines.append, groundtruth=None)
    except tritd.TritdError as e:
        assert e.status == NODEV, e  # no GPU here: the solver was reached, and it is the first call
        out = None
    assert spy.used and spy.used[0] == "triple_decomp_ADMM_outlier"
    assert not [n for n in spy.used if "foreground" in n]
    if out is not None:  # with a GPU: what the driver printed and returned before
        assert len(lines) == 2 and lines[1].startswith("TRIPLE ADMM - RMSE:")
        assert not {"precision", "recall", "f1", "pwc", "fg_counts", "fg_mask"} & set(out)
