"""Inputs of the NaN-as-missing tests (observed="nan", opts.nanmissing):
the existing masked goldens with NaN written at their unobserved entries, and
the mock-gateway callers.  Shared by tests/test_nan_missing.py (CPU) and
tests/test_gpu_nan_missing.py (GPU).

The NaNs are written through an integer view, so numpy never quiets them: a
positive and a negative quiet NaN, one with a payload and a signalling one.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import PKG, ROOT

MOCK = os.path.join(ROOT, "tests", "mock_mex")
NAN_BITS = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000123,
                     0x7ff0000000000001], dtype=np.uint64)
ADMM_FIELDS = ["mu", "rho", "lambda", "lambda2", "maxIter", "tol", "disp"]


def with_nans(D, observed):
    """where(observed, D, NaN), column-major, the NaNs cycling through NAN_BITS
    in column-major order of the missing entries."""
    Dn = np.array(D, dtype=np.float64, order="F", copy=True)
    bits = Dn.reshape(-1, order="F").view(np.uint64)  # (a view of Dn: it is column-major)
    assert np.shares_memory(bits, Dn)
    idx = np.flatnonzero(~np.asarray(observed, dtype=bool).reshape(-1, order="F"))
    bits[idx] = NAN_BITS[np.arange(idx.size) % NAN_BITS.size]
    assert np.array_equal(~np.isnan(Dn), np.asarray(observed, dtype=bool))
    assert idx.size < NAN_BITS.size or {int(b) for b in bits[idx]} == {int(b) for b in NAN_BITS}
    return Dn


def as_single(D):
    with np.errstate(invalid="ignore"):  # (casting the signalling NaN raises the invalid flag)
        return np.asfortranarray(D, dtype=np.float32)


def holdout_with_flags_outside(holdout, observed, count=3):
    """The golden's H plus `count` flags at unobserved entries (which hold NaN
    in the test input): only H & Omega counts, so nothing may change."""
    H = np.array(holdout, dtype=bool, order="F", copy=True)
    idx = np.flatnonzero(~np.asarray(observed, dtype=bool).reshape(-1, order="F"))
    flat = H.reshape(-1, order="F")
    flat[idx[:: max(1, idx.size // count)][:count]] = True
    assert (H & ~observed).sum() >= min(count, idx.size)
    return H


def build_gateway(tmp_path_factory):
    """matlab/tritd_mex.cpp against the mock mx runtime, as tests/test_mex_gateway.py builds it."""
    out = tmp_path_factory.mktemp("mex_nan") / "libmexmock.so"
    libdir = os.path.join(PKG, "tritd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + MOCK,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(PKG, "matlab", "tritd_mex.cpp"), os.path.join(MOCK, "mock_mex.cpp"),
                    "-L" + libdir, "-ltritd", "-Wl,-rpath," + libdir, "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.mock_admm.restype = C.c_int
    lib.mock_als.restype = C.c_int
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _err_hist(names, vals):
    """The errHist buffer of a gateway call: the gateway returns up to the
    maxIter it is GIVEN (in vals), so the buffer is sized by that."""
    mi = int(vals[list(names).index("maxIter")]) if "maxIter" in names else 0
    return np.zeros(max(mi, 0) + 1)


def gateway_admm(gw, g, D, names, vals, single=False):
    D = as_single(D) if single else np.asfortranarray(D, dtype=np.float64)
    n1, n2, n3 = D.shape
    r = g["r"]
    vals = np.array(vals, dtype=np.float64)
    A = np.zeros((n1, r, r), order="F")
    B = np.zeros((r, n2, r), order="F")
    Cc = np.zeros((r, r, n3), order="F")
    O, E = np.zeros_like(D), np.zeros_like(D)
    eh = _err_hist(names, vals)
    k = C.c_int(0)
    err, pr = C.create_string_buffer(1024), C.create_string_buffer(4096)
    A0, B0, C0 = (np.asfortranarray(g[x]) for x in ("A0", "B0", "C0"))
    rc = gw.mock_admm(_p(D), n1, n2, n3, r, ",".join(names).encode(), _p(vals), _p(A0), _p(B0),
                      _p(C0), _p(A), _p(B), _p(Cc), _p(O), _p(E), _p(eh), C.byref(k), err, 1024, pr,
                      4096, int(single))
    return rc, err.value.decode(), dict(A=A, B=B, C=Cc, O=O, E=E, errHist=eh[: k.value], k=k.value)


def gateway_als(gw, g, X, names, vals):
    X = np.asfortranarray(X, dtype=np.float64)
    n1, n2, n3 = X.shape
    r = g["r"]
    vals = np.array(vals, dtype=np.float64)
    A = np.zeros((n1, r, r), order="F")
    B = np.zeros((r, n2, r), order="F")
    Cc = np.zeros((r, r, n3), order="F")
    eh = _err_hist(names, vals)
    k = C.c_int(0)
    err, pr = C.create_string_buffer(1024), C.create_string_buffer(4096)
    A0, B0, C0 = (np.asfortranarray(g[x]) for x in ("A0", "B0", "C0"))
    rc = gw.mock_als(_p(X), n1, n2, n3, r, ",".join(names).encode(), _p(vals), _p(A0), _p(B0),
                     _p(C0), _p(A), _p(B), _p(Cc), _p(eh), C.byref(k), err, 1024, pr, 4096)
    return rc, err.value.decode(), dict(A=A, B=B, C=Cc, errHist=eh[: k.value], k=k.value)
