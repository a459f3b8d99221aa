"""The truncated-pinv fallback (csrc/pinv.h) at every padded rank and in every
consumer, against the CPU references of tests/pinv_cases.py.

tests/test_gpu_flags.py reaches the fallback at RP = 16 only (6 x 2 x 2,
r = 3, update_A).  The cases here are rank deficient on purpose (tests/
test_pinv_cases.py shows on the CPU that every Gram they meet is cleanly
truncated or well conditioned, that two CPU references agree to 1e-10 and that
an inverse in pinv's place lands >= 1e-5 away), and reach:

  group      solver         request (solve)            consumer
  A_small    ADMM fp64      k_solve_ns<16|32|48|64>    k_apply<16|32|48|64> (A, 3 workgroups)
  A_rows     ADMM fp64      k_solve_ns<16|48|64>       k_apply<16|48|64> (A, 7..88 workgroups,
                                                       each redoing the Jacobi in LDS)
  A_wide     ADMM fp64      k_solve_mw<128|256>        k_pinv_fix<128|256> (global scratch)
  C_trunc    ADMM fp64 x2   side solve in K2 (sweep.h) k_apply<32|64|16> (C), k_pinv_fix<128|256>
                            / k_solve_mw               on the solve's stream; the second solve
                                                       starts from a replaced inverse
  ABC_trunc  ADMM, ALS x2   ns<16> / side solves       A (after the stop test), B (YT ==
                                                       nullptr) and C
  ALS        ALS x2         k_solve_ns<16|32|48|64>    k_apply<..> of als.cpp (A; C)
  F32        ADMM single    ns<16|64>, mw<128|256>     k_pinv_fix<16|64|128|256> (LDS / global)
  optional   Qi ADMM (k_apply<48>), nonconvex solver (als.cpp, ridge 1e-12)
  devset     set_devices([0, 0]), TRITD_SHOV=0         k_apply_gram<16|32|48|64> for A, C and
                                                       (ABC) B: the phase-serial order is the
                                                       one schedule that takes the
                                                       one-workgroup apply+Gram; by default
                                                       the fused sharded iteration (k_apply)
(kernel names from a kernel trace of one case per group: on one GPU the fused
iteration defers the Gram of a small factor to a side solve and applies
through k_apply, so k_apply_gram runs for device sets in the phase-serial
order only.)

Every call warns (PinvToleranceWarning) and raises TRITD_FLAG_PINV_TOL; k is the
reference's.  fp64: rel L and rel A, B, C <= 1e-8 (the min-norm factors are
unique: the sharpest witness that the truncation happened); where the fit is
not exact rel O, rel E (or E identically zero) and errHist (relative) <= 1e-8;
where it is (C truncates: errHist ~1e-15, O rounding noise)
||O - O_ref|| / ||X||, likewise E, and |d errHist| <= 1e-8.  float32:
test_gpu_f32._compare (TOL = 2e-5 and its errHist bound).  Two-iteration cases
also run stepped 1 + 1 through Session / AlsSession, bitwise equal to the
one-shot call; one E-active control per RP class raises no flag.

Out of scope: spectra with values between 0.5 x and 1e6 x the cutoff, so the
cutoff constant itself is pinned no better than the cleanest margin (0.13 x ..
0.16 x at (2, 2, 40) r = 3).

Measured on an MI355X (every case passes; `worst` the largest of the compared
figures and where, against the 1e-8 bound; wall time of the one-shot call):
  case              RP   worst             s     case              RP   worst             s
  A_small_r4        16   9.7e-15 (A)             C_trunc_r5        32   1.3e-14 (C)
  A_small_r5        32   6.1e-15 (A)             C_trunc_r8        64   9.8e-14 (C)
  A_small_r6        48   5.1e-15 (A)             C_trunc_r8_rows   64   1.1e-13 (C)
  A_small_r7        64   5.9e-15 (L)             C_trunc_r4_rows   16   1.4e-13 (B)
  A_small_r8        64   6.7e-15 (L)             C_trunc_r9       128   2.1e-12 (B)    0.30
  A_rows_r4         16   1.7e-13 (C)             C_trunc_r16      256   2.2e-12 (C)    6.1
  A_rows_r8         64   5.7e-15 (O)             ABC_trunc_admm    16   2.0e-12 (C)
  A_rows_r6         48   9.8e-15 (O)             ABC_trunc_als     16   9.6e-13 (B)
  A_wide_r9        128   6.9e-15 (L)   0.16      ALS_A_r6          48   1.7e-09 (errHist)
  A_wide_r11       128   5.3e-15 (L)   0.12      ALS_A_r8          64   3.7e-10 (errHist)
  A_wide_r12       256   1.2e-14 (L)   0.88      ALS_C_r4 / r5 / r8     2.0e-13 / 1.2e-14 / 8.5e-14
  A_wide_r16       256   1.2e-14 (L)   3.1       opt_qi_r6         48   4.3e-15 (L)
  devset_* (SHOV=0, k_apply_gram) 16..64: as the one-GPU cases (9.7e-15 .. 9.7e-14; ABC 3.6e-12)
  opt_ncvx_r6       48   5.3e-13 (A)
  F32_r4 / r8 / r9 / r16: rel L 1.9e-7 / 1.5e-7 / 1.5e-7 / 1.2e-7, rel O <= 2.0e-7 (TOL 2e-5),
  errHist <= 0.8 % of its bound; F32_r16 3.1 s.
(the RP <= 64 cases take 0.01 .. 0.06 s.)  ALS_A_*: X is fitted to ~1e-6, so the
relative errHist amplifies the rounding of L (3e-14) by ~1e6: 1.7e-9 is
rounding, not truncation error (tests/pinv_cases.py _SEEDS).

The one-workgroup Jacobi in global memory: one fallback takes ~0.1 s at
RP = 128 (k_pinv_fix<128> 104 ms in a kernel trace, R = 81, 56 values dropped)
and ~3 s at RP = 256 (R = 256, 192 dropped: 3.1 s per iteration of A_wide_r16,
F32_r16 and C_trunc_r16, whose two iterations and stepped session take 6.1 s
each; R = 144: 0.9 s).  Rare by construction, and not tuned here.
"""
import time
import warnings

import numpy as np
import pytest

import pinv_cases as pc
import sweep_cases as sc
from test_gpu_f32 import _compare

pytestmark = pytest.mark.gpu

TOL = pc.TOL64


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def cref():
    return sc.cref_lib()


def _params(names):
    """RP = 128 / 256 run the one-workgroup Jacobi in global memory: a time limit."""
    return [pytest.param(n, marks=pytest.mark.timeout(120)) if pc.rp_class(pc.CASES[n]) > 64 else n
            for n in names]


_ONE_SHOT = {}


def one_shot(tritd, name, tag=""):
    """The one-shot call of a fp64 case inside pytest.warns: (result dict,
    flags, seconds).  Kept per process (and per `tag`, the caller's schedule
    switch) for the session comparison."""
    if (name, tag) in _ONE_SHOT:
        return _ONE_SHOT[name, tag]
    from tritd import _lib
    case = pc.CASES[name]
    X, r, A0, B0, C0, opts = pc.inputs(case)
    if case.devices:
        tritd.set_devices(list(case.devices))
    t0 = time.time()
    try:
        with pytest.warns(tritd.PinvToleranceWarning):
            if case.solver == "als":
                A, B, C, eh, k = tritd.triple_decomp_ALS(X, r, opts, A0, B0, C0, return_iters=True)
                got = dict(A=A, B=B, C=C, errHist=eh, k=k)
            elif case.solver == "ncvx":
                A, B, C, O, eh, k = tritd.triple_decomp_ncvx(X, r, *sc.ncvx_args(opts), A0, B0, C0,
                                                             return_iters=True)
                got = dict(A=A, B=B, C=C, O=O, errHist=eh, k=k)
            else:
                A, B, C, O, eh, E, k = tritd.triple_decomp_ADMM(X, r, opts, A0, B0, C0,
                                                                return_E=True, return_iters=True)
                got = dict(A=A, B=B, C=C, O=O, E=E, errHist=eh, k=k)
        flags = _lib.lib.tritd_last_flags()
    finally:
        if case.devices:
            tritd.set_devices([])
    _ONE_SHOT[name, tag] = (got, flags, time.time() - t0)
    return _ONE_SHOT[name, tag]


def check(tritd, capsys, name, tag=""):
    from tritd import _lib
    ref = pc.reference(name)
    got, flags, secs = one_shot(tritd, name, tag)
    f = pc.figures(name, got, ref)
    with capsys.disabled():
        print("  pinv %-16s RP %3d k=%d (ref %d) flags=%#x %.2f s  %s"
              % (name + tag, pc.padded_rank(pc.CASES[name].r), got["k"], ref["k"], flags, secs,
                 {k: float("%.2g" % v) for k, v in f.items()}), flush=True)
    assert got["k"] == ref["k"] == len(got["errHist"])
    assert flags & _lib.FLAG_PINV_TOL
    assert max(f.values()) <= TOL, f


@pytest.mark.parametrize("name", _params(pc.names("A_small", "A_rows", "A_wide")))
def test_admm_update_A_truncates(tritd, capsys, name):
    check(tritd, capsys, name)


@pytest.mark.parametrize("name", _params(pc.names("C_trunc")))
def test_admm_update_C_truncates_two_iterations(tritd, capsys, name):
    check(tritd, capsys, name)


@pytest.mark.parametrize("name", pc.names("ABC_trunc"))
def test_every_update_truncates(tritd, capsys, name):
    check(tritd, capsys, name)


@pytest.mark.parametrize("name", pc.names("ALS"))
def test_als_truncates(tritd, capsys, name):
    check(tritd, capsys, name)


@pytest.mark.parametrize("name", pc.names("optional"))
def test_optional_cases(tritd, capsys, name):
    check(tritd, capsys, name)


@pytest.mark.parametrize("name,shov", [(n, "0") for n in pc.names("devset")]
                         + [("devset_r6", "1"), ("devset_C_r5", "1")])
def test_device_set_truncates(tritd, capsys, monkeypatch, name, shov):
    """set_devices([0, 0]).  TRITD_SHOV=0, the phase-serial order: small factors
    go through the one-workgroup apply+Gram, k_apply_gram<16|32|48|64> for A
    (devset_r*), for C (devset_C_*) and for A, B (YT == nullptr) and C
    (devset_ABC_r3), pA | pV sharing LDS with the Y chunk.  Default: the fused
    sharded iteration (k_apply; A's Gram a side job of M2)."""
    monkeypatch.setenv("TRITD_SHOV", shov)
    check(tritd, capsys, name, " SHOV=" + shov)


@pytest.mark.parametrize("name", _params(pc.names("F32")))
def test_class_single_truncates(tritd, cref, capsys, name):
    from tritd import _lib
    case = pc.CASES[name]
    X, r, A0, B0, C0, opts = pc.inputs(case)
    assert X.dtype == np.float32
    ref = pc.reference(name)
    ref = (ref["A"], ref["B"], ref["C"], ref["O"], ref["errHist"], ref["E"], ref["k"])
    rep = {}
    t0 = time.time()
    try:
        with pytest.warns(tritd.PinvToleranceWarning):
            _compare(tritd, cref, X, r, opts, A0, B0, C0, ref=ref, report=rep)
    finally:
        with capsys.disabled():
            print("  pinv %-16s RP %3d %.2f s  %s"
                  % (name, pc.padded_rank(r), time.time() - t0,
                     {k: (float("%.3g" % v) if isinstance(v, float) else v) for k, v in rep.items()}),
                  flush=True)
    assert _lib.lib.tritd_last_flags() & _lib.FLAG_PINV_TOL


# one stepped session per RP class (<= 64, 128, 256) and solver
@pytest.mark.parametrize("name", _params(["C_trunc_r5", "C_trunc_r9", "C_trunc_r16", "ABC_trunc_admm",
                                          "ABC_trunc_als", "ALS_A_r6"]))
def test_stepped_session_is_bitwise_the_one_shot_call(tritd, capsys, name):
    from tritd import _lib
    case = pc.CASES[name]
    assert case.iters == 2
    X, r, A0, B0, C0, opts = pc.inputs(case)
    n1, n2, n3 = case.shape
    got = one_shot(tritd, name)[0]
    t0 = time.time()
    if case.solver == "als":
        s = tritd.AlsSession(r, opts, A0, B0, C0, n1=n1, n2=n2, n3=n3, X=X, device=0)
        keys = ("A", "B", "C", "errHist")
    else:
        s = tritd.Session(r, opts, A0, B0, C0, n1=n1, n2=n2, n3=n3, D=X, device=0, probe=False)
        keys = ("A", "B", "C", "O", "E", "errHist")
    try:
        s.run(1)
        s.run(1)
        s.sync()
        flags = s.flags()
        with pytest.warns(tritd.PinvToleranceWarning):
            res = s.get()
    finally:
        s.close()
    with capsys.disabled():
        print("  pinv session %-16s flags=%#x k=%d %.2f s" % (name, flags, res["k"], time.time() - t0),
              flush=True)
    assert flags & _lib.FLAG_PINV_TOL
    assert res["k"] == got["k"] == 2
    for key in keys:
        np.testing.assert_array_equal(res[key], got[key], err_msg=key)


@pytest.mark.parametrize("r", [6, pytest.param(11, marks=pytest.mark.timeout(120)),
                               pytest.param(16, marks=pytest.mark.timeout(120))])
def test_well_conditioned_control_raises_no_flag(tritd, r):
    """The flag of the cases above is not set unconditionally: the E-active
    sweep case of the same RP class (48, 128, 256), 2 iterations."""
    from tritd import _lib
    c = sc.e_active_case(r)
    with warnings.catch_warnings():
        warnings.simplefilter("error", tritd.PinvToleranceWarning)
        tritd.triple_decomp_ADMM(c["D"], r, dict(c["opts"], maxIter=2), c["A0"], c["B0"], c["C0"])
    assert (_lib.lib.tritd_last_flags() & _lib.FLAG_PINV_TOL) == 0
