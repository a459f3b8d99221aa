"""Mask-aware fp64 ADMM on the GPU at every rank with an ACTIVE outlier tensor E.

The masked goldens (tests/test_gpu_masked.py) reach r in {2, 3, 5, 7, 8, 12}
and, with the traffic options, compare an E that is identically zero for the
first 12-20 iterations.  Here every masked k5_fused instantiation that
launch_k5 (csrc/k_admm.hip) can select runs tests/masked_sweep_cases.py: the CP
model at r = 1..16 (padded rank 16, 32, 48, 64, 128, 256, with and without rank
padding inside it) and the Qi model at r = 1..8, ragged shapes of about
36 x 21 x 34, 10 iterations, 15 % of the entries missing plus a wholly missing
tile, a ragged edge tile with no observed real row and a fully observed tile;
nnz(E) is 5..71 % of the observed entries, split between compact slots and
dense tiles (asserted on the CPU by tests/test_masked_sweep_cases.py, with the
admission rule of the masked goldens).

Reference: tests/masked_oracle.py.  Comparison: test_gpu_masked.check_masked at
the tolerances of tests/masked_cases.py, unchanged (L, O, E <= 1e-9; A, B, C <=
1e-8; errHist rtol 1e-8 atol 1e-11; same k; O and E exactly 0 where nothing
was observed).

One rank per instantiation, r in {1, 5, 6, 7, 11, 13} (SCHEDULE_RANKS), also
runs through a Session stepped 3 + 7 (whose dense-tile counter shows both
storage forms occurred), the split t-walk, a device set of one GPU three times
(shards of 11-13 rows straddling the 16-row tiles) and a one-rank RCCL
communicator; the padded ranks <= 64 (NARROW) also the side-stream schedule
(TRITD_FUSED=0) and the dense-E form (k5_profile() == (7, 0)).  Qi r = 6 takes
the k_w_reduce path of the split walk and the device set.  cp r = 3, 6, 11 run
with a mask that hides every row of shard 0 of three.

Measured on an MI355X (one-shot call; worst of the schedules in brackets; nnz(E)
as a share of the observed entries; errHist in units of its gate, 1e-8 |ref| +
1e-11):
  case    nnz(E)   L        O        E        A        B        C        errHist(gate)
  cp-r1   0.133  1.1e-15  6.3e-16  6.1e-16  3.3e-15  1.7e-15  4.5e-15  1.7e-07  [L,O,E 1.6e-15; A,B,C 6.3e-15]
  cp-r2   0.050  4.8e-15  2.0e-15  6.7e-16  5.3e-15  3.4e-15  6.6e-15  7.8e-07
  cp-r3   0.104  6.3e-15  3.9e-15  2.6e-15  6.4e-15  4.8e-15  6.9e-15  3.5e-07
  cp-r4   0.051  4.4e-15  2.0e-15  9.0e-16  7.2e-15  5.4e-15  4.2e-15  9.7e-08
  cp-r5   0.433  2.7e-14  1.3e-14  1.2e-14  3.7e-14  3.5e-14  2.6e-14  4.8e-07  [L,O,E 2.9e-14; A,B,C 3.8e-14]
  cp-r6   0.472  1.1e-14  7.2e-15  6.9e-15  1.7e-14  1.6e-14  1.9e-14  4.5e-08  [L,O,E 1.2e-14; A,B,C 2.0e-14]
  cp-r7   0.569  1.5e-14  9.7e-15  9.6e-15  1.7e-14  1.7e-14  1.9e-14  4.6e-08  [L,O,E 1.5e-14; A,B,C 2.0e-14]
  cp-r8   0.643  1.3e-14  8.8e-15  9.0e-15  1.2e-14  1.1e-14  1.2e-14  6.1e-08
  cp-r9   0.650  1.9e-14  1.4e-14  1.4e-14  1.6e-14  1.5e-14  1.7e-14  8.3e-08
  cp-r10  0.626  1.8e-14  1.7e-14  1.7e-14  1.6e-14  1.3e-14  1.6e-14  4.9e-08
  cp-r11  0.616  2.1e-14  2.3e-14  2.3e-14  1.8e-14  1.5e-14  1.8e-14  3.0e-08  [L,O,E 2.3e-14; A,B,C 1.9e-14]
  cp-r12  0.561  2.4e-14  3.4e-14  3.4e-14  2.2e-14  1.8e-14  2.2e-14  1.4e-07
  cp-r13  0.540  2.5e-14  4.0e-14  4.0e-14  2.2e-14  1.8e-14  2.3e-14  4.0e-08  [L,O,E 4.0e-14; A,B,C 2.3e-14]
  cp-r14  0.506  2.6e-14  4.8e-14  4.8e-14  2.4e-14  2.0e-14  2.4e-14  7.7e-08
  cp-r15  0.330  2.6e-14  8.6e-14  8.4e-14  2.9e-14  2.1e-14  2.9e-14  8.2e-08
  cp-r16  0.206  2.4e-14  1.1e-13  1.1e-13  3.0e-14  2.2e-14  3.0e-14  2.2e-07
  qi-r1   0.133  8.3e-16  4.1e-16  3.6e-16  2.0e-15  5.9e-15  8.1e-15  2.0e-07
  qi-r2   0.577  1.6e-14  1.0e-14  1.1e-14  1.2e-14  1.4e-14  1.9e-14  1.9e-07
  qi-r3   0.058  3.3e-15  1.5e-15  7.3e-16  5.0e-15  4.4e-15  3.6e-15  2.7e-07
  qi-r4   0.162  7.3e-15  6.8e-15  5.3e-15  9.3e-15  1.1e-14  6.9e-15  6.3e-07
  qi-r5   0.679  1.1e-14  7.1e-15  7.3e-15  1.1e-14  1.2e-14  1.3e-14  4.8e-08
  qi-r6   0.695  1.2e-14  7.3e-15  7.4e-15  1.1e-14  1.0e-14  1.3e-14  5.9e-08  [L,O,E 1.2e-14; A,B,C 1.4e-14]
  qi-r7   0.709  1.7e-14  9.8e-15  1.0e-14  1.5e-14  1.3e-14  1.5e-14  1.5e-07
  qi-r8   0.697  1.5e-14  9.5e-15  9.7e-15  1.3e-14  1.1e-14  1.3e-14  3.7e-08
The hidden-shard masks (three shards and one device): L, O, E <= 3.1e-14; A, B,
C <= 3.2e-14; errHist <= 5.4e-07 of its gate.
Dense-tile totals of the 3 + 7 sessions (of 10 launches x tiles per launch):
r=1 297 of 1800, r=5 580 of 1800, r=6 554 of 1800, r=7 723 of 1920,
r=11 815 of 1800, r=13 597 of 2040.
No test here exposed a fault of the masked kernels.
"""
import numpy as np
import pytest

import masked_sweep_cases as ms
import sweep_cases as sc
from test_gpu_masked import check_masked

pytestmark = pytest.mark.gpu

IDS = [ms.case_id(c) for c in ms.CASES]
CP_SCHEDULE = [("cp", r) for r in ms.SCHEDULE_RANKS]
CP_NARROW = [("cp", r) for r in ms.NARROW]
WITH_QI6 = CP_SCHEDULE + [("qi", 6)]
HIDDEN = [("cp", r) for r in ms.HIDDEN_RANKS]


def ids(cases):
    return [ms.case_id(c) for c in cases]


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


def solve(tritd, g, **kw):
    return tritd.triple_decomp_ADMM(g["D"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"], return_E=True,
                                    return_iters=True, **dict(dict(observed=g["observed"]), **kw))


def session(tritd, g, comm=None):
    n1, n2, n3 = g["D"].shape
    return tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3, D=g["D"],
                         device=0, comm=comm, probe=False, observed=g["observed"])


def session_result(s):
    x = s.get()
    return x["A"], x["B"], x["C"], x["O"], x["errHist"], x["E"], x["k"]


def check(orc, got, g, what):
    """check_masked, after the share of E that is nonzero and a guard that the
    comparison is not one of two zero tensors."""
    print("  masked sweep %s %s nnz(E)/nnz(observed)=%.3f" %
          (g["name"], what, ms.nnz_of_observed(got[5], g["observed"])), flush=True)
    assert np.any(g["E"]) and np.any(got[5])
    check_masked(orc, got, g, g["name"], what)


# --- 1. one-shot: every masked instantiation, CP and Qi ---------------------------
@pytest.mark.parametrize("case", ms.CASES, ids=IDS)
def test_one_shot(tritd, orc, case):
    g = ms.golden_like(case)
    check(orc, solve(tritd, g), g, "one-shot")


# --- 2. sessions ---------------------------------------------------------------------
@pytest.mark.parametrize("case", CP_SCHEDULE, ids=ids(CP_SCHEDULE))
def test_session_uneven_steps_and_both_storage_forms(tritd, orc, case):
    """3 + 7 iterations; the dense-tile counter shows that compact slots and
    dense tiles both occurred (0 < dense total < launches x tiles)."""
    g = ms.golden_like(case)
    s = session(tritd, g)
    try:
        assert s.mask_info() == (True, int(g["observed"].sum()))
        s.run(3)
        s.run(7)
        got = session_result(s)
        dense, per = s.counters()
    finally:
        s.close()
    check(orc, got, g, "session 3+7")
    print("  masked sweep %s dense tiles %d of %d x %d" % (g["name"], dense, ms.ITERS, per), flush=True)
    assert 0 < dense < ms.ITERS * per


# --- 3. schedules and storage forms -------------------------------------------------
@pytest.mark.parametrize("case", CP_NARROW, ids=ids(CP_NARROW))
def test_side_stream_schedule(tritd, orc, case, monkeypatch):
    monkeypatch.setenv("TRITD_FUSED", "0")
    g = ms.golden_like(case)
    check(orc, solve(tritd, g), g, "TRITD_FUSED=0")


@pytest.mark.parametrize("case", CP_NARROW, ids=ids(CP_NARROW))
def test_dense_e_form(tritd, orc, case, monkeypatch):
    monkeypatch.setenv("TRITD_DENSE_E", "1")
    g = ms.golden_like(case)
    check(orc, solve(tritd, g), g, "TRITD_DENSE_E=1")
    s = session(tritd, g)
    try:
        s.run(1)
        s.sync()
        assert s.k5_profile() == (7, 0)  # dense E streams, no slot accesses: the form really ran
        assert s.mask_info()[0]
    finally:
        s.close()


@pytest.mark.parametrize("case", WITH_QI6, ids=ids(WITH_QI6))
def test_split_t_walk(tritd, orc, case, monkeypatch):
    monkeypatch.setenv("TRITD_K5_TSPLIT", "2")
    g = ms.golden_like(case)
    check(orc, solve(tritd, g), g, "TRITD_K5_TSPLIT=2")


# --- 4. shards ------------------------------------------------------------------------
def solve_on_three(tritd, g):
    tritd.set_devices([0, 0, 0])
    try:
        return solve(tritd, g)
    finally:
        tritd.set_devices([])


@pytest.mark.parametrize("case", WITH_QI6, ids=ids(WITH_QI6))
def test_device_set(tritd, orc, case):
    g = ms.golden_like(case)
    check(orc, solve_on_three(tritd, g), g, "set_devices([0,0,0])")


def test_device_set_phase_serial(tritd, orc, monkeypatch):
    monkeypatch.setenv("TRITD_SHOV", "0")
    g = ms.golden_like(("cp", 6))
    check(orc, solve_on_three(tritd, g), g, "set_devices([0,0,0]) TRITD_SHOV=0")


@pytest.mark.parametrize("case", CP_SCHEDULE, ids=ids(CP_SCHEDULE))
def test_rccl_one_rank(tritd, orc, case):
    g = ms.golden_like(case)
    comm = tritd.Comm(tritd.Comm.unique_id(), 1, 0, 0)
    try:
        s = session(tritd, g, comm)
        try:
            s.run(ms.ITERS)
            got = session_result(s)
        finally:
            s.close()
    finally:
        comm.close()
    check(orc, got, g, "rccl one rank")


@pytest.mark.parametrize("case", HIDDEN, ids=ids(HIDDEN))
def test_a_shard_with_nothing_observed(tritd, orc, case):
    """Shard 0 of three observes nothing while the others do: the observed
    count rides in the norm all-reduce, so every shard still sees a mask with
    observed entries.  The same mask on one device is the control."""
    H = ms.hidden_shard_mask(case)
    assert not H[:H.shape[0] // 3].any() and H[H.shape[0] // 3:].any()
    g = ms.golden_like(case, H, ms.hidden_reference(case))
    check(orc, solve_on_three(tritd, g), g, "hidden shard, set_devices([0,0,0])")
    check(orc, solve(tritd, g), g, "hidden shard, one device")


# --- 5. oracle-free invariants ------------------------------------------------------
@pytest.mark.parametrize("r", [6, 10, 16])
def test_all_true_mask_is_the_unmasked_call_bitwise(tritd, r):
    g = ms.inputs(("cp", r))
    ref = solve(tritd, g, observed=None)
    got = solve(tritd, g, observed=np.ones(g["D"].shape, dtype=bool))
    assert np.any(ref[5]) and len(got) == len(ref) == 7 and got[6] == ref[6]
    for a, b in zip(got[:6], ref[:6]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("r", [6, 10, 16])
def test_fill_values_never_enter(tritd, r):
    g = ms.inputs(("cp", r))
    miss = ~g["observed"]
    D0 = g["D"].copy(order="F")
    D0[miss] = 0.0
    ref = solve(tritd, dict(g, D=D0))
    assert np.any(ref[5])
    for fill in (np.nan, 1e30):
        D = g["D"].copy(order="F")
        D[miss] = fill
        got = solve(tritd, dict(g, D=D))
        assert got[6] == ref[6]
        for a, b in zip(got[:6], ref[:6]):
            np.testing.assert_array_equal(a, b)


# --- 6. device-resident D and mask ----------------------------------------------------
@pytest.mark.parametrize("r", [6, 11])
def test_session_with_device_mask_and_padded_leading_dimension(tritd, orc, r):
    """D and the mask resident on the device, ldD = n1 + 5 (elements of D,
    bytes of the mask), the padding rows holding NaN / 0xFF bytes."""
    from tritd import hip
    g = ms.golden_like(("cp", r))
    n1, n2, n3 = g["D"].shape
    ld = n1 + 5
    Dp = np.full((ld, n2, n3), np.nan, order="F")
    Dp[:n1] = g["D"]
    Mp = np.full((ld, n2, n3), 0xFF, dtype=np.uint8, order="F")
    Mp[:n1] = g["observed"]
    dD, dM = hip.DeviceArray.from_host(Dp), hip.DeviceArray.from_host(Mp)
    try:
        s = tritd.Session(r, g["opts"], g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3,
                          d_device_ptr=dD.ptr, ldD=ld, device=0, probe=False, observed=dM.ptr)
    finally:
        dD.free()
        dM.free()
    try:
        assert s.mask_info() == (True, int(g["observed"].sum()))
        s.run(ms.ITERS)
        got = session_result(s)
    finally:
        s.close()
    check(orc, got, g, "device D and mask, ldD = n1 + 5")
