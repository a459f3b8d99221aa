"""fp64 ADMM on the GPU at every rank r = 1..16 with an ACTIVE outlier tensor E.

The goldens cover r in {1,2,3,5,8,10,12,16}, and outside the r <= 8 goldens
their E is identically zero (tests/sweep_cases.py explains why).  Here every
rank — every padded rank RP in {16, 32, 48, 64, 128, 256}, with and without
rank padding inside it — runs tests/sweep_cases.e_active_case: ragged shapes
of about 35 x 20 x 33, 10 iterations, nnz(E) 13..63 % split between compact
slots and dense tiles (asserted on the CPU by tests/test_sweep_cases.py, which
also shows the oracle and the C restatement agree to 3e-13 on these inputs).

Reference: the numpy oracle.  Tolerances: those of tests/test_gpu_parity.py,
unchanged (L, O, E <= 1e-9; A, B, C <= 1e-8; errHist rtol 1e-8 atol 1e-11;
same k).

One rank per kernel instantiation, r in {4, 6, 7, 11, 13} (RP = 16 unpadded,
48, 64 padded, 128, 256), also runs through a Session stepped 3 + 7, the
side-stream schedule (TRITD_FUSED=0), the dense-E form, the split t-walk,
three virtual shards (12-13 rows each, straddling the 16-row tiles), a device
set of one GPU twice, and a one-rank RCCL communicator.

The tall case (sweep_cases.TALL: 97 x 83 x 85 at r = 7) runs the same forms
past the one-launch threshold of apply + Gram, where every factor update is
an apply and a Gram launch and no Gram is deferred to a side job: one-shot and
3 + 7 on the fused schedule, the side-stream schedule, three virtual shards
(32 / 32 / 33 rows: A^ small again, its Gram a side job of M2), the device set
on the fused schedule and on the phase functions (TRITD_SHOV=0), and the
one-rank communicator on the fused and on the side-stream schedule.

Measured on an MI355X (one-shot call; worst of the schedules in brackets):
   r  nnz(E)   L        O        E        A        B        C        errHist(rel)
   1  0.127  3.1e-15  2.0e-15  1.9e-15  1.1e-14  3.9e-14  3.0e-14  2.2e-15
   2  0.158  2.5e-14  3.0e-14  2.8e-14  2.0e-14  2.1e-14  1.3e-14  1.0e-13
   3  0.249  3.1e-15  1.6e-15  1.3e-15  8.4e-15  5.8e-15  6.4e-15  2.3e-15
   4  0.216  4.3e-15  2.2e-15  1.8e-15  8.4e-15  6.4e-15  7.3e-15  1.0e-15  [L,O,E 4.3e-15; A,B,C 8.4e-15]
   5  0.201  1.3e-14  8.9e-15  7.3e-15  1.8e-14  2.3e-14  2.3e-14  2.7e-15
   6  0.298  8.5e-14  4.3e-14  3.4e-14  5.8e-14  1.2e-13  8.9e-14  5.6e-15  [L,O,E 8.5e-14; A,B,C 1.2e-13]
   7  0.417  1.5e-14  9.5e-15  8.7e-15  1.4e-14  2.0e-14  1.8e-14  7.2e-16  [L,O,E 1.8e-14; A,B,C 2.6e-14]
   8  0.561  2.4e-14  1.6e-14  1.5e-14  2.8e-14  2.7e-14  3.2e-14  9.4e-16
   9  0.634  2.2e-14  1.6e-14  1.6e-14  2.2e-14  2.0e-14  2.4e-14  2.8e-16
  10  0.630  2.4e-14  2.0e-14  2.0e-14  2.3e-14  1.8e-14  2.3e-14  9.6e-16
  11  0.617  2.7e-14  2.6e-14  2.6e-14  2.6e-14  2.1e-14  2.7e-14  7.7e-16  [L,O,E 2.7e-14; A,B,C 2.7e-14]
  12  0.598  2.9e-14  3.7e-14  3.6e-14  2.7e-14  2.3e-14  2.8e-14  4.3e-16
  13  0.578  2.9e-14  4.2e-14  4.2e-14  2.8e-14  2.3e-14  2.9e-14  1.2e-15  [L,O,E 4.3e-14; A,B,C 2.9e-14]
  14  0.556  3.1e-14  5.1e-14  5.1e-14  3.1e-14  2.5e-14  3.0e-14  5.7e-16
  15  0.430  3.2e-14  9.7e-14  9.5e-14  3.9e-14  2.8e-14  4.2e-14  8.8e-16
  16  0.336  2.8e-14  1.2e-13  1.2e-13  4.1e-14  2.9e-14  4.1e-14  2.1e-15
tall  0.168  5.9e-15  2.8e-15  1.7e-15  2.0e-14  2.3e-14  2.4e-14  4.0e-15  [L,O,E 5.9e-15; A,B,C 2.4e-14]
Dense-tile totals of the 3 + 7 sessions (of 10 launches x tiles per launch):
r=4 241 of 2160, r=6 547 of 1800, r=7 698 of 1920, r=11 904 of 1800, r=13 726 of 2040,
tall 5470 of 35040.
"""
import numpy as np
import pytest

import sweep_cases as sc
from conftest import rel
from test_gpu_parity import ATOL_ERR, TOL_ABC, TOL_ERR, TOL_LOE

pytestmark = pytest.mark.gpu

SCHEDULE_RANKS = [4, 6, 7, 11, 13]
NARROW = [r for r in SCHEDULE_RANKS if r * r <= 64]  # padded rank <= 64
TALL = [sc.TALL]


def with_env(cases, var):
    """(case, None) under the ids the bare cases had, then the tall case with var=0."""
    return ([pytest.param(c, None, id=str(c)) for c in cases + TALL]
            + [pytest.param(sc.TALL, var, id="tall-%s=0" % var)])


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


def check(orc, got, case, label, ref=None, e_zero=False, model="cp"):
    """check_solution of test_gpu_parity.py, printing each figure before it asserts.
    ref: another reference than the sweep's own for `case` (tests/test_gpu_opts_ladder.py);
    e_zero: E is identically zero on both sides where the caller's options make it so."""
    if ref is None:
        ref = sc.oracle_ref(case)
    A, B, C, O, eh, E, k = got
    dev = dict(L=rel(orc.triple_product(A, B, C, model),
                     orc.triple_product(ref["A"], ref["B"], ref["C"], model)),
               O=rel(O, ref["O"]), E=rel(E, ref["E"]), A=rel(A, ref["A"]), B=rel(B, ref["B"]),
               C=rel(C, ref["C"]))
    n = min(len(eh), len(ref["errHist"]))
    dev["eh"] = float(np.max(np.abs(eh[:n] - ref["errHist"][:n]) / ref["errHist"][:n])) if n else 0.0
    print("  sweep r=%s %s k=%d nnz(E)=%.3f " % (case, label, k, sc.nnz_share(E))
          + " ".join("%s=%.1e" % kv for kv in dev.items()), flush=True)
    assert k == ref["k"] and len(eh) == ref["k"]
    if e_zero:
        assert not np.any(ref["E"]) and not np.any(E)
    else:
        assert np.any(ref["E"]) and np.any(E)
    assert dev["L"] <= TOL_LOE and dev["O"] <= TOL_LOE and dev["E"] <= TOL_LOE, dev
    assert dev["A"] <= TOL_ABC and dev["B"] <= TOL_ABC and dev["C"] <= TOL_ABC, dev
    np.testing.assert_allclose(eh, ref["errHist"], rtol=TOL_ERR, atol=ATOL_ERR)


def solve(tritd, case, **kw):
    c = sc.e_active_case(case)
    return tritd.triple_decomp_ADMM(c["D"], c["r"], c["opts"], c["A0"], c["B0"], c["C0"],
                                    return_E=True, return_iters=True, **kw)


def session(tritd, case, comm=None):
    c = sc.e_active_case(case)
    n1, n2, n3 = c["D"].shape
    return tritd.Session(c["r"], c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                         D=c["D"], device=0, comm=comm)


def session_result(s):
    x = s.get()
    return x["A"], x["B"], x["C"], x["O"], x["errHist"], x["E"], x["k"]


@pytest.mark.parametrize("r", sc.RANKS + (sc.TALL,))
def test_one_shot(tritd, orc, r):
    check(orc, solve(tritd, r), r, "one-shot")


@pytest.mark.parametrize("r", SCHEDULE_RANKS + TALL)
def test_session_uneven_steps_and_both_storage_forms(tritd, orc, r):
    """3 + 7 iterations; the dense-tile counter shows that compact slots and
    dense tiles both occurred (0 < dense total < launches x tiles)."""
    s = session(tritd, r)
    try:
        s.run(3)
        s.run(7)
        got = session_result(s)
        dense, per = s.counters()
    finally:
        s.close()
    check(orc, got, r, "session 3+7")
    print("  sweep r=%s dense tiles %d of %d x %d" % (r, dense, sc.ITERS, per), flush=True)
    assert 0 < dense < sc.ITERS * per


@pytest.mark.parametrize("r", NARROW + TALL)
def test_side_stream_schedule(tritd, orc, r, monkeypatch):
    monkeypatch.setenv("TRITD_FUSED", "0")
    check(orc, solve(tritd, r), r, "TRITD_FUSED=0")


@pytest.mark.parametrize("r", NARROW)
def test_dense_e_form(tritd, orc, r, monkeypatch):
    monkeypatch.setenv("TRITD_DENSE_E", "1")
    check(orc, solve(tritd, r), r, "TRITD_DENSE_E=1")
    s = session(tritd, r)
    try:
        s.run(1)
        s.sync()
        assert s.k5_profile() == (7, 0)  # dense E streams, no slot accesses: the form really ran
    finally:
        s.close()


@pytest.mark.parametrize("r", SCHEDULE_RANKS)
def test_split_t_walk(tritd, orc, r, monkeypatch):
    monkeypatch.setenv("TRITD_K5_TSPLIT", "2")
    check(orc, solve(tritd, r), r, "TRITD_K5_TSPLIT=2")


@pytest.mark.parametrize("r", SCHEDULE_RANKS + TALL)
def test_virtual_shards(tritd, orc, r):
    check(orc, solve(tritd, r, virtual_shards=3), r, "virtual_shards=3")


@pytest.mark.parametrize("r, shov", with_env(SCHEDULE_RANKS, "TRITD_SHOV"))
def test_device_set(tritd, orc, r, shov, monkeypatch):
    """TRITD_SHOV=0: the two shards run the phase functions, not the fused schedule."""
    if shov is not None:
        monkeypatch.setenv("TRITD_SHOV", "0")
    tritd.set_devices([0, 0])
    try:
        got = solve(tritd, r)
    finally:
        tritd.set_devices([])
    check(orc, got, r, "set_devices([0,0])" + (" TRITD_SHOV=0" if shov else ""))


@pytest.mark.parametrize("r, fused", with_env(SCHEDULE_RANKS, "TRITD_FUSED"))
def test_rccl_one_rank(tritd, orc, r, fused, monkeypatch):
    """TRITD_FUSED=0: the side-stream schedule with its all-reduces."""
    if fused is not None:
        monkeypatch.setenv("TRITD_FUSED", "0")
    comm = tritd.Comm(tritd.Comm.unique_id(), 1, 0, 0)
    try:
        s = session(tritd, r, comm)
        try:
            s.run(sc.ITERS)
            got = session_result(s)
        finally:
            s.close()
    finally:
        comm.close()
    check(orc, got, r, "rccl one rank" + (" TRITD_FUSED=0" if fused else ""))
