"""The boundary of a Session: how D gets in, how O / E get out, and
tritd_session_rre_parts — the calls bench.py and a multi-GPU host make
(device-resident D with a leading dimension, a pointer to D(i0,0,0) of the
whole tensor) and the source of the bench line's rre_final / rre_vs_cpu.

Inputs: tests/boundary_cases.py (sweep_cases.e_active_case at one rank per
padded rank 16 .. 256, fp32 at r = 4, 16, the Qi model at r = 2, 5, 8, and
the three degenerate shapes with a singleton mode), 3 + 7 iterations, every
session created with probe=False.  tests/test_boundary_cases.py holds the CPU
conditions on them.

1. Five ways of handing over D — host contiguous (a), host with ldD = n1 + 3
   (b), device contiguous (c), device strided (d), device pointer to row 3 of
   a buffer of n1 + 5 rows (e; only element-aligned) — every element outside
   the shard NaN, the caller's device buffer freed (and its memory reused for
   NaNs) straight after creation.  (a) against the oracle at the tolerances
   of the module that owns the path (test_gpu_rank_sweep.check, test_gpu_f32,
   test_gpu_als, test_gpu_parity's degenerate cases); (b)-(e) bitwise equal
   to (a) in A, B, C, O, E, errHist and k.
   AlsSession: the ALS kernels stop at r = 8 (include/tritd.h,
   TRITD_ERR_UNSUPPORTED above), so r = 11 cannot be solved: at r = 11 every
   form must return that status, and the parity of the five forms runs at
   r = 4 and r = 7 (padded rank 16 unpadded and 64 padded).
2. A proper sub-range [5, n1 - 4) without a communicator IS the standalone
   problem D[i0:i1], A0[i0:i1], B0, C0: the constructor packs A0's rows
   i0..i1-1, norm(D) is the shard's, and Session::allreduce returns at once.
   Created from D(i0,0,0) of the whole device tensor with ldD = n1; get()
   writes rows i0..i1-1 of A only.
3. tritd_session_get / _f32 with ldOE = n1l + 3: rows < n1l bitwise the
   contiguous get(), the other rows untouched; ldOE = n1l - 1 and a create
   with ldD < i1 - i0 return TRITD_ERR_ARG and write nothing.
4. rre_parts(X, ldX) against a float64 restatement on the session's OWN
   factors (the kernel, not the iterates): num = sum (L - X)^2, den = sum X^2
   for X1 = Lstar, X2 independent normal, X3 = L (1 + 1e-6 U) in the three
   buffer forms, after 3 + 7 iterations and on a fresh session.  Tolerances
   (boundary_cases.rre_reference): den rtol 1e-12; num rtol
   1e-12 + 2e-13 |L| / |L - X| computed from the reference.  A NaN means a
   padded element was read.
   (Sharded sums over ranks: tests/test_gpu_dist_host.py.)

Measured on an MI355X: relative deviation of num for X1, X2 (tolerance
1.1e-12 .. 1.9e-12) and X3 (tolerance 1.6e-7 .. 4.0e-7) and of den (1e-12),
worst over the three buffer forms and fresh / iterated; the three forms gave
the same bits in every case.
  case         num X1   num X2   num X3   den
  cp4         2.3e-16  4.0e-16  4.6e-12  2.6e-16
  cp5         1.1e-16  1.2e-16  8.4e-12  3.4e-16
  cp6         0.0e+00  2.7e-16  4.0e-12  2.4e-16
  cp8         0.0e+00  1.4e-16  4.3e-12  1.9e-16
  cp11        2.2e-16  1.4e-16  4.5e-12  2.1e-16
  cp16        0.0e+00  1.7e-16  8.1e-12  2.4e-16
  f324        3.1e-16  2.7e-16  4.0e-12  2.6e-16
  f3216       1.5e-16  0.0e+00  5.9e-12  3.2e-16
  qi2         4.1e-16  3.0e-16  1.3e-11  2.0e-16
  qi5         2.0e-16  1.9e-16  1.3e-12  4.1e-16
  qi8         1.4e-16  1.5e-16  1.7e-11  3.6e-16
  deg5x1x7    3.7e-16  1.4e-16  2.1e-10  4.0e-16
  deg1x9x8    2.0e-16  1.9e-16  1.1e-10  3.6e-16
  deg33x17x1  1.9e-16  2.1e-16  2.4e-11  2.0e-16
Form (a) against its reference: fp64 the figures of test_gpu_rank_sweep.py's
table (r = 16: O, E 1.2e-13); fp32 L, O, E <= 1.5e-7 (r = 4), 4.8e-6
(r = 16); degenerate shapes <= 3.2e-14; ALS A, B, C <= 1.2e-14.  Forms
(b)-(e) gave the bits of (a) everywhere.
With a library whose k_to_tm / k_to_tm32 read the source with the shard's
row count in place of ld, items 1 and 2 fail in all 15 cases; with one whose
rre_parts passes the row count as the stride of X, all 28 cases of item 4 fail.
"""
import ctypes as C

import numpy as np
import pytest

import boundary_cases as bc
import sweep_cases as sc
from conftest import rel
from test_gpu_parity import check_solution

pytestmark = pytest.mark.gpu

TRITD_ERR_ARG = 1
TRITD_ERR_UNSUPPORTED = 7
FORMS5 = [("host", "contig"), ("host", "strided"), ("device", "contig"), ("device", "strided"),
          ("device", "offset")]
KEYS = ("A", "B", "C", "O", "E", "errHist")
IDS = [bc.case_id(c) for c in bc.CASES]
SOLVE_CASES = [c for c in bc.CASES if c[0] != "qi"]
SENTINEL = {np.dtype(np.float64): -1.2345e300, np.dtype(np.float32): -1.2345e30}


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def hip(tritd):
    from tritd import hip as h
    return h


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


class Uploaded:
    """A padded buffer on the device; `.ptr` is the shard's first element."""

    def __init__(self, hip, X, form):
        self.hip = hip
        self.host, self.ld, off = bc.padded(X, form)
        self.dev = hip.DeviceArray.from_host(self.host)
        self.ptr = self.dev.ptr + off * self.host.itemsize
        self.poison = None

    def free(self, reuse=False):
        """reuse: hand the freed memory to a buffer of NaNs that lives on, so
        a session still reading the caller's D would show it."""
        self.dev.free()
        if reuse:
            self.poison = self.hip.DeviceArray.from_host(np.full_like(self.host, np.nan))

    def close(self):
        self.dev.free()
        if self.poison is not None:
            self.poison.free()


def open_session(tritd, hip, case, where="host", form="contig", als=False):
    """-> (session, Uploaded or None); the caller's device buffer is freed already."""
    c = bc.inputs(case)
    n1, n2, n3 = c["D"].shape
    kw = dict(n1=n1, n2=n2, n3=n3, device=0)
    args = (c["r"], sc.ALS_OPTS if als else c["opts"], c["A0"], c["B0"], c["C0"])
    up = None
    if where == "device":
        up = Uploaded(hip, c["D"], form)
        try:
            if als:
                s = tritd.AlsSession(*args, x_device_ptr=up.ptr, ldX=up.ld, **kw)
            else:
                s = tritd.Session(*args, d_device_ptr=up.ptr, ldD=up.ld, dtype=up.host.dtype,
                                  probe=False, **kw)
        except Exception:
            up.close()
            raise
        up.free(reuse=True)
    else:
        buf, ld, off = bc.padded(c["D"], form)
        assert off == 0
        if als:
            s = tritd.AlsSession(*args, X=buf, ldX=ld, **kw)
        else:
            s = tritd.Session(*args, D=buf, ldD=ld, probe=False, **kw)
    return s, up


def solve(tritd, hip, case, where="host", form="contig", als=False):
    s, up = open_session(tritd, hip, case, where, form, als)
    try:
        for n in bc.STEPS:
            s.run(n)
        return s.get()
    finally:
        s.close()
        if up is not None:
            up.close()


def rre_all(hip, s, case, fresh):
    """{(x, form): (num, den)} of the session for the three X in the three forms"""
    out = {}
    for x, X in enumerate(bc.rre_tensors(case, fresh)):
        for form in bc.FORMS:
            up = Uploaded(hip, X, form)
            try:
                out[x, form] = s.rre_parts(up.ptr, up.ld)
            finally:
                up.close()
    return out


_BASE = {}


def baseline(tritd, hip, case):
    """Form (a) of a case, once per process: its get() after 3 + 7 iterations
    with the rre parts of that state, and the factors and rre parts of a fresh
    session."""
    if case not in _BASE:
        out = {}
        s, _ = open_session(tritd, hip, case)
        try:
            out["rre", True] = rre_all(hip, s, case, True)
            out["get", True] = s.get()
        finally:
            s.close()
        s, _ = open_session(tritd, hip, case)
        try:
            for n in bc.STEPS:
                s.run(n)
            out["get", False] = s.get()
            out["rre", False] = rre_all(hip, s, case, False)
        finally:
            s.close()
        _BASE[case] = out
    return _BASE[case]


def as_tuple(x):
    return x["A"], x["B"], x["C"], x["O"], x["errHist"], x["E"], x["k"]


def check_f32(orc, got, case):
    """_compare of test_gpu_f32.py on a session's result, its tolerances unchanged."""
    from test_gpu_f32 import TOL, check_errhist
    ref, c = bc.reference(case), bc.inputs(case)
    assert got["O"].dtype == np.float32 and got["E"].dtype == np.float32 and got["A"].dtype == np.float64
    Lr = orc.triple_product(ref["A"], ref["B"], ref["C"])
    dev = dict(L=rel(orc.triple_product(got["A"], got["B"], got["C"]), Lr),
               O=rel(got["O"].astype(np.float64), ref["O"].astype(np.float64)),
               E=rel(got["E"].astype(np.float64), ref["E"].astype(np.float64)))
    print("  boundary %s (a): k=%d " % (bc.case_id(case), got["k"])
          + " ".join("%s=%.1e" % kv for kv in dev.items()), flush=True)
    assert got["k"] == ref["k"] and np.any(ref["E"])
    assert max(dev.values()) <= TOL, dev
    check_errhist(got["errHist"], ref["errHist"], c["D"], Lr, ref["O"], ref["E"])


def check_degenerate(orc, got, case):
    """_degenerate of test_gpu_parity.py on a session's result, its tolerances unchanged."""
    ref = bc.reference(case)
    dev = dict(L=rel(orc.triple_product(got["A"], got["B"], got["C"]),
                     orc.triple_product(ref["A"], ref["B"], ref["C"])),
               O=rel(got["O"], ref["O"]), E=rel(got["E"], ref["E"]))
    print("  boundary %s (a): k=%d " % (bc.case_id(case), got["k"])
          + " ".join("%s=%.1e" % kv for kv in dev.items()), flush=True)
    assert got["k"] == ref["k"] and np.any(ref["E"]) and np.any(got["E"])
    assert max(dev.values()) <= 1e-8, dev
    np.testing.assert_allclose(got["errHist"], ref["errHist"], rtol=1e-7, atol=1e-11)


def assert_same_bits(got, base, label):
    assert got["k"] == base["k"], label
    for key in KEYS:
        assert got[key].dtype == base[key].dtype and got[key].shape == base[key].shape, (label, key)
        np.testing.assert_array_equal(got[key], base[key], err_msg="%s: %s" % (label, key))


# ---------------------------------------------------------------------------
# 1. every way of handing D to a session gives bitwise the same solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", SOLVE_CASES, ids=[bc.case_id(c) for c in SOLVE_CASES])
def test_every_way_of_handing_over_D_is_the_same_solve(tritd, hip, orc, case):
    base = baseline(tritd, hip, case)["get", False]
    assert base["k"] == bc.ITERS and not any(np.isnan(base[k]).any() for k in KEYS)
    if case[0] == "cp":
        from test_gpu_rank_sweep import check
        check(orc, as_tuple(base), case[1], "boundary (a)")
    elif case[0] == "f32":
        check_f32(orc, base, case)
    else:
        check_degenerate(orc, base, case)
    forms = FORMS5[1:] if case[0] != "deg" else [FORMS5[1], FORMS5[4]]
    for where, form in forms:
        assert_same_bits(solve(tritd, hip, case, where, form), base, "%s %s" % (where, form))


@pytest.mark.parametrize("r", [4, 7])
def test_every_way_of_handing_over_X_is_the_same_als(tritd, hip, orc, r):
    from test_gpu_als import check
    case = ("cp", r)
    base = solve(tritd, hip, case, als=True)
    ref = sc.oracle_als_ref(r)
    print("  boundary ALS r=%d (a): A %.1e B %.1e C %.1e" % (
        r, rel(base["A"], ref[0]), rel(base["B"], ref[1]), rel(base["C"], ref[2])), flush=True)
    check(orc, (base["A"], base["B"], base["C"], base["errHist"], base["k"]), *ref)
    for where, form in FORMS5[1:]:
        got = solve(tritd, hip, case, where, form, als=True)
        assert got["k"] == base["k"]
        for key in ("A", "B", "C", "errHist"):
            np.testing.assert_array_equal(got[key], base[key], err_msg="%s %s: %s" % (where, form, key))


def test_als_session_refuses_r11_in_every_form(tritd, hip):
    """The ALS path is r <= 8: no form of X may get past that."""
    for where, form in FORMS5:
        with pytest.raises(tritd.TritdError) as e:
            open_session(tritd, hip, ("cp", 11), where, form, als=True)[0].close()
        assert e.value.status == TRITD_ERR_UNSUPPORTED, (where, form)


# ---------------------------------------------------------------------------
# raw C-ABI calls: what tritd.Session cannot express (ldOE, a pre-filled A)
# ---------------------------------------------------------------------------
def raw_get(s, ldOE):
    """tritd_session_get(_f32) into sentinel-filled buffers.  -> (status, dict):
    O, E as (ldOE, n2, n3) views of their buffers (element (i,j,t) at
    i + ldOE (j + n2 t)), tailO / tailE the elements of the buffers behind
    that extent, k = -7 where the call left it alone."""
    from tritd._lib import lib
    dt = np.dtype(np.float32 if s.f32 else np.float64)
    s64 = SENTINEL[np.dtype(np.float64)]
    nl, r, plane = s.i1 - s.i0, s.r, s.n2 * s.n3
    out = dict(A=np.full((s.n1, r, r), s64, order="F"), B=np.full((r, s.n2, r), s64, order="F"),
               C=np.full((r, r, s.n3), s64, order="F"), errHist=np.full(max(s.maxIter, 1), s64))
    flat = {key: np.full((max(ldOE, nl) + 3) * plane, SENTINEL[dt], dtype=dt) for key in ("O", "E")}
    k = C.c_int32(-7)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    fn = lib.tritd_session_get_f32 if s.f32 else lib.tritd_session_get
    st = fn(s._s, p(out["A"]), p(out["B"]), p(out["C"]), p(flat["O"]), p(flat["E"]), int(ldOE),
            p(out["errHist"]), C.byref(k))
    for key in ("O", "E"):
        out[key] = flat[key][:ldOE * plane].reshape((ldOE, s.n2, s.n3), order="F")
        out["tail" + key] = flat[key][ldOE * plane:]
    out["k"] = k.value
    return st, out


def untouched(a):
    a = np.asarray(a)
    return bool(np.all(a == SENTINEL[a.dtype]))


# ---------------------------------------------------------------------------
# 2. a proper sub-range without a communicator is the standalone sub-problem
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("r", bc.SUB_RANKS)
def test_sub_range_without_communicator_is_the_standalone_problem(tritd, hip, orc, r):
    c = sc.e_active_case(r)
    n1, n2, n3 = c["D"].shape
    i0, i1 = bc.sub_range(n1)
    full = hip.DeviceArray.from_host(c["D"])  # the whole tensor; the session gets D(i0,0,0)
    try:
        s = tritd.Session(r, c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3, i0=i0, i1=i1,
                          d_device_ptr=full.ptr + 8 * i0, ldD=n1, device=0, probe=False)
    finally:
        full.free()
    try:
        for n in bc.STEPS:
            s.run(n)
        st, got = raw_get(s, i1 - i0)
    finally:
        s.close()
    assert st == 0
    assert untouched(got["A"][:i0]) and untouched(got["A"][i1:]) and not np.any(
        got["A"][i0:i1] == SENTINEL[np.dtype(np.float64)])
    assert untouched(got["tailO"]) and untouched(got["tailE"])
    ref = bc.sub_reference(r)
    k = got["k"]
    check_solution(orc, (np.asfortranarray(got["A"][i0:i1]), got["B"], got["C"], got["O"],
                         got["errHist"][:k], got["E"], k), ref, ref["k"])
    assert np.any(got["E"])


# ---------------------------------------------------------------------------
# 3. get with ldOE > i1 - i0; argument errors write nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("cp", 4), ("cp", 11), ("f32", 16), ("deg", 2)],
                         ids=["cp4", "cp11", "f32_16", "deg33x17x1"])
def test_get_with_a_leading_dimension(tritd, hip, case):
    s, _ = open_session(tritd, hip, case)
    try:
        for n in bc.STEPS:
            s.run(n)
        base = s.get()
        nl = s.i1 - s.i0
        st, got = raw_get(s, nl + 3)
        st_bad, bad = raw_get(s, nl - 1)
        again = s.get()
    finally:
        s.close()
    assert st == 0 and got["k"] == base["k"] == bc.ITERS
    for key in ("O", "E"):
        assert got[key].dtype == base[key].dtype and np.any(base[key])
        np.testing.assert_array_equal(got[key][:nl], base[key], err_msg=key)
        assert untouched(got[key][nl:]) and untouched(got["tail" + key]), key
    for key in ("A", "B", "C"):
        np.testing.assert_array_equal(got[key], base[key], err_msg=key)
    np.testing.assert_array_equal(got["errHist"][:got["k"]], base["errHist"])
    assert st_bad == TRITD_ERR_ARG and bad["k"] == -7
    for key in ("A", "B", "C", "O", "E", "errHist", "tailO", "tailE"):
        assert untouched(bad[key]), key
    assert_same_bits(again, base, "get() after the strided and the refused get")


@pytest.mark.parametrize("kind", ["cp", "f32"])
def test_create_refuses_a_leading_dimension_below_the_shard(tritd, hip, kind):
    from tritd._lib import SESSION_D_ON_DEVICE, SESSION_F32, lib
    from tritd.api import make_opts
    c = bc.inputs((kind, 4))
    n1, n2, n3 = c["D"].shape
    o = make_opts(c["opts"])
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    f32 = SESSION_F32 if c["f32"] else 0
    dev = hip.DeviceArray.from_host(c["D"])
    try:
        for dptr, flags in ((p(c["D"]), f32), (C.c_void_p(dev.ptr), f32 | SESSION_D_ON_DEVICE)):
            for i0, i1 in ((0, n1), (5, n1 - 4)):
                h = C.c_void_p(0x1234)
                st = lib.tritd_session_create(C.byref(h), 0, dptr, i1 - i0 - 1, n1, n2, n3, i0, i1, 4,
                                              C.byref(o), p(c["A0"]), p(c["B0"]), p(c["C0"]), None, flags)
                assert st == TRITD_ERR_ARG and not h.value
                assert b"ldD" in lib.tritd_last_error()
    finally:
        dev.free()


# ---------------------------------------------------------------------------
# 4. rre_parts against a float64 restatement on the session's own factors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fresh", [False, True], ids=["iterated", "fresh"])
@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_rre_parts_against_float64_restatement(tritd, hip, orc, case, fresh):
    base = baseline(tritd, hip, case)
    f, c = base["get", fresh], bc.inputs(case)
    if fresh:
        assert f["k"] == 0
        for key in ("A", "B", "C"):
            np.testing.assert_array_equal(f[key], c[key + "0"])
    else:
        assert f["k"] == bc.ITERS
    L = orc.triple_product(f["A"], f["B"], f["C"], model=c["model"])
    rows, bad = [], []
    for x, X in enumerate(bc.rre_tensors(case, fresh)):
        num_ref, den_ref, rtol_num, rtol_den = bc.rre_reference(L, X)
        for form in bc.FORMS:
            num, den = base["rre", fresh][x, form]
            dn, dd = abs(num - num_ref) / num_ref, abs(den - den_ref) / den_ref
            rows.append("X%d %-7s num %.17g (ref %.17g) dev %.1e of %.1e | den dev %.1e of %.1e"
                        % (x + 1, form, num, num_ref, dn, rtol_num, dd, rtol_den))
            if not (np.isfinite(num) and np.isfinite(den) and dn <= rtol_num and dd <= rtol_den):
                bad.append(rows[-1])
    print("  rre_parts %s %s\n    " % (bc.case_id(case), "fresh" if fresh else "iterated")
          + "\n    ".join(rows), flush=True)
    assert not bad, bad
    # the three buffer forms hold the same X: the same sums to the last bit
    for x in range(3):
        assert len({base["rre", fresh][x, form] for form in bc.FORMS}) == 1, x
