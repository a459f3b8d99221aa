"""Which C symbol each form of the Python front end reaches first
(tritd/api.py: the one-shot functions and the session constructors).  A
recording wrapper stands in for ``tritd.api.lib`` and forwards to the real
library, so on a host without a GPU every call ends in TRITD_ERR_NODEV (caught
here) after it has been recorded, and with a GPU it runs: 6 x 5 x 4, r = 2."""
import numpy as np
import pytest

import tritd
from tritd import _lib, api, synth

N1, N2, N3, R = 6, 5, 4, 2
OPTS = dict(synth.TRAFFIC_OPTS, maxIter=3)
NCVX = dict(rho=1.1, lam=0.5, gamma_A=1e-3, epsilon=1e-3, p=0.5, theta=1.0)


class Recorder:
    """``tritd.api.lib`` with the name of every tritd_* call kept in order"""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("tritd_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


@pytest.fixture()
def rec(monkeypatch):
    r = Recorder(api.lib)
    monkeypatch.setattr(api, "lib", r)
    return r


@pytest.fixture(scope="module")
def data():
    d = synth.low_rank_plus_outliers(N1, N2, N3, R, seed=5)
    rng = np.random.default_rng(11)
    d["observed"] = np.asfortranarray(rng.random((N1, N2, N3)) < 0.8)
    d["holdout"] = np.asfortranarray(rng.random((N1, N2, N3)) < 0.2)
    d["Dnan"] = np.where(d["observed"], d["D"], np.nan)
    d["start"] = (d["A0"], d["B0"], d["C0"])
    return d


def first_symbol(rec, fn, *args, **kw):
    """The first C symbol ``fn(*args, **kw)`` reaches; a missing device is no failure."""
    del rec.calls[:]
    try:
        out = fn(*args, **kw)
        if hasattr(out, "close"):
            out.close()
    except tritd.TritdError as e:
        assert e.status == 6, e  # TRITD_ERR_NODEV alone
    assert rec.calls, "no C call was made"
    return rec.calls[0]


ONE_SHOT = [
    ("ADMM", {}, "tritd_admm_f64"),
    ("ADMM", dict(observed="array"), "tritd_admm_masked_f64"),
    ("ADMM", dict(observed="nan"), "tritd_admm_masked_f64"),
    ("ADMM", dict(holdout="array"), "tritd_admm_holdout_f64"),
    ("ADMM", dict(holdout="array", observed="array"), "tritd_admm_holdout_f64"),
    ("ADMM", dict(virtual_shards=2), "tritd_admm_sharded_virtual_f64"),
    ("ADMM", dict(f32=True), "tritd_admm_f32"),
    ("ALS", {}, "tritd_als_f64"),
    ("ALS", dict(observed="array"), "tritd_als_masked_f64"),
    ("ALS", dict(holdout="array"), "tritd_als_holdout_f64"),
    ("ALS", dict(virtual_shards=2), "tritd_als_sharded_virtual_f64"),
    ("ncvx", {}, "tritd_ncvx_f64"),
    ("ncvx", dict(observed="array"), "tritd_ncvx_masked_f64"),
    ("ncvx", dict(holdout="array"), "tritd_ncvx_holdout_f64"),
]


def _keywords(kw, data):
    """the table's keywords with the arrays put in; -> (D, keywords)"""
    kw = dict(kw)
    D = data["D"].astype(np.float32) if kw.pop("f32", False) else data["D"]
    if kw.get("observed") == "nan":
        D = data["Dnan"]
    for name in ("observed", "holdout"):
        if kw.get(name) == "array":
            kw[name] = data[name]
    return D, kw


def _ids(table):
    return ["%s-%s" % (name, "+".join("%s=%s" % kv for kv in sorted(kw.items())) or "plain")
            for name, kw, _ in table]


@pytest.mark.parametrize("solver,kw,symbol", ONE_SHOT, ids=_ids(ONE_SHOT))
def test_one_shot_reaches_its_symbol(rec, data, solver, kw, symbol):
    D, kw = _keywords(kw, data)
    if solver == "ADMM":
        got = first_symbol(rec, tritd.triple_decomp_ADMM, D, R, OPTS, *data["start"], **kw)
    elif solver == "ALS":
        got = first_symbol(rec, tritd.triple_decomp_ALS, D, R, OPTS, *data["start"], **kw)
    else:
        got = first_symbol(rec, tritd.triple_decomp_ncvx, D, R, NCVX["rho"], NCVX["lam"],
                           NCVX["gamma_A"], NCVX["epsilon"], NCVX["p"], NCVX["theta"], 3, 1e-6,
                           *data["start"], **kw)
    assert got == symbol


SESSIONS = [
    ("Session", {}, "tritd_session_create"),
    ("Session", dict(observed="array"), "tritd_session_create_masked"),
    ("Session", dict(holdout="array"), "tritd_session_create_holdout"),
    ("AlsSession", {}, "tritd_als_session_create"),
    ("AlsSession", dict(observed="array"), "tritd_als_session_create_masked"),
    ("AlsSession", dict(holdout="array"), "tritd_als_session_create_holdout"),
    ("NcvxSession", dict(holdout="array"), "tritd_als_session_create_ncvx_holdout"),
]


@pytest.mark.parametrize("cls,kw,symbol", SESSIONS, ids=_ids(SESSIONS))
def test_session_reaches_its_creator(rec, data, cls, kw, symbol):
    D, kw = _keywords(kw, data)
    where = dict(n1=N1, n2=N2, n3=N3, device=0)
    if cls == "Session":
        got = first_symbol(rec, tritd.Session, R, OPTS, *data["start"], D=D, probe=False, **where,
                           **kw)
    elif cls == "AlsSession":
        got = first_symbol(rec, tritd.AlsSession, R, OPTS, *data["start"], X=D, **where, **kw)
    else:
        got = first_symbol(rec, tritd.NcvxSession, R, OPTS, *data["start"], X=D, ncvx=NCVX,
                           **where, **kw)
    assert got == symbol


def test_float32_with_a_mask_is_refused_before_any_c_call(rec, data):
    D32 = data["D"].astype(np.float32)
    for kw in (dict(observed=data["observed"]), dict(holdout=data["holdout"]), dict(observed="nan")):
        with pytest.raises(tritd.TritdError) as e:
            tritd.triple_decomp_ADMM(D32, R, OPTS, *data["start"], **kw)
        assert e.value.status == _lib.TRITD_ERR_UNSUPPORTED
    assert rec.calls == []


def test_a_string_mask_other_than_nan_is_a_value_error(rec, data):
    D, start = data["D"], data["start"]
    with pytest.raises(ValueError):
        tritd.triple_decomp_ADMM(D, R, OPTS, *start, holdout="nan")
    with pytest.raises(ValueError):
        tritd.triple_decomp_ADMM(D, R, OPTS, *start, observed="NaN")
    with pytest.raises(ValueError):
        tritd.triple_decomp_ALS(D, R, OPTS, *start, holdout="nan")
    with pytest.raises(ValueError):
        tritd.triple_decomp_ncvx(D, R, *(NCVX[k] for k in ("rho", "lam", "gamma_A", "epsilon", "p", "theta")),
                                 3, 1e-6, *start, observed="NaN")
    with pytest.raises(ValueError):
        tritd.AlsSession(R, OPTS, *start, n1=N1, n2=N2, n3=N3, X=D, holdout="nan")
    assert rec.calls == []
