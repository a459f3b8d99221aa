"""GPU parity: libtritd (HIP, gfx950) against the oracle on the same inputs.

Tolerances (fp64; BASELINE.json north_star "within a stated fp64 tolerance"):
  * L = triple_product(A,B,C), O, E : relative Frobenius <= 1e-9
  * A, B, C                         : relative Frobenius <= 1e-8
  * errHist                         : |d| <= 1e-8*errHist + 1e-11 entrywise, same k
    (errHist is ||resL||/||D|| + ||resO||/||D||; resL = D - L - O cancels, so
    its rounding floor is ~eps in units of ||D||, hence the absolute floor)
  * data-movement primitives (unfold, buildF/G/H, soft_threshold): bit-exact
The GPU and the oracle differ only in summation order and in inverse-vs-pinv
of well-conditioned R x R Grams (<= 1.4e-11 after 100 its).
"""
import numpy as np
import pytest

from conftest import golden_names, load_golden, rel

pytestmark = pytest.mark.gpu

TOL_LOE = 1e-9
TOL_ABC = 1e-8
TOL_ERR = 1e-8
ATOL_ERR = 1e-11


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def orc():
    import tritd_oracle
    return tritd_oracle


def check_solution(orc, got, ref, k_ref):
    A, B, C, O, eh, E, k = got
    assert k == k_ref
    assert len(eh) == k_ref
    L = orc.triple_product(A, B, C)
    Lr = orc.triple_product(ref["A"], ref["B"], ref["C"])
    assert rel(L, Lr) <= TOL_LOE
    assert rel(O, ref["O"]) <= TOL_LOE
    assert rel(E, ref["E"]) <= TOL_LOE
    for key, X in (("A", A), ("B", B), ("C", C)):
        assert rel(X, ref[key]) <= TOL_ABC, key
    np.testing.assert_allclose(eh, ref["errHist"], rtol=TOL_ERR, atol=ATOL_ERR)


@pytest.mark.parametrize("name", golden_names())
def test_admm_matches_golden(tritd, orc, name):
    g = load_golden(name)
    got = tritd.triple_decomp_ADMM(g["D"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                   return_E=True, return_iters=True)
    check_solution(orc, got, g, g["k"])


@pytest.mark.parametrize("name,env", [
    # dense-E form of K5 from the first iteration (solver.cpp de_mode_)
    ("g12x10x8_r2", {"TRITD_DENSE_E": "1"}), ("g12x10x8_r2_stop", {"TRITD_DENSE_E": "1"}),
    ("g17x16x20_r8", {"TRITD_DENSE_E": "1"}), ("g20x24x18_r5_video", {"TRITD_DENSE_E": "1"}),
    ("g30_r3", {"TRITD_DENSE_E": "1"}), ("g54x4x96_r5_sensor", {"TRITD_DENSE_E": "1"}),
    # the t-walk cut into chunks whose partial W sets k_w_reduce sums (k5_tsplit)
    ("g17x16x20_r8", {"TRITD_K5_TSPLIT": "2"}), ("g30_r3", {"TRITD_K5_TSPLIT": "2"}),
    ("g20x24x18_r5_video", {"TRITD_K5_TSPLIT": "2"}), ("g54x4x96_r5_sensor", {"TRITD_K5_TSPLIT": "3"}),
    ("g54x4x96_r5_sensor", {"TRITD_K5_TSPLIT": "3", "TRITD_DENSE_E": "1"}),
])
def test_admm_storage_forms_match_golden(tritd, orc, name, env, monkeypatch):
    """K5's other storage/decomposition forms (dense E, split t-walk), forced
    on the goldens: the same solution within the same tolerances."""
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    g = load_golden(name)
    got = tritd.triple_decomp_ADMM(g["D"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                   return_E=True, return_iters=True)
    check_solution(orc, got, g, g["k"])
    if "TRITD_DENSE_E" in env:  # the form really ran: K5 reports dense E streams, no slots
        n1, n2, n3 = g["D"].shape
        s = tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3, D=g["D"],
                          device=0)
        s.run(1)
        s.sync()
        assert s.k5_profile() == (7, 0)
        s.close()


@pytest.mark.parametrize("name", ["g12x10x8_r2", "g30_r3", "g17x16x20_r8"])
def test_admm_first_iterations(tritd, orc, name):
    """State after iterations 1 and 2 (localises a divergence)."""
    g = load_golden(name)
    for it in (1, 2):
        opts = dict(g["opts"], maxIter=it)
        A, B, C, O, eh, k = tritd.triple_decomp_ADMM(g["D"], g["r"], opts, g["A0"], g["B0"], g["C0"],
                                                     return_iters=True)
        assert k == it
        for key, X in (("A", A), ("B", B), ("C", C)):
            assert rel(X, g[f"it{it}_{key}"]) <= 1e-11, (it, key)


@pytest.mark.parametrize("name,P", [("g30_r3", 2), ("g30_r3", 3), ("g54x4x96_r5_sensor", 4),
                                    ("g17x16x20_r8", 2)])
def test_virtual_shards_match_golden(tritd, orc, name, P):
    """Mode-1 sharded schedule rehearsed as P shards on one GPU."""
    g = load_golden(name)
    got = tritd.triple_decomp_ADMM(g["D"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                   return_E=True, return_iters=True, virtual_shards=P)
    check_solution(orc, got, g, g["k"])


@pytest.mark.parametrize("name,P,serial", [("g30_r3", 3, False), ("g54x4x96_r5_sensor", 2, False),
                                           ("g17x16x20_r8", 3, False), ("g12x10x8_r2_stop", 2, False),
                                           ("g30_r3", 3, True), ("g54x4x96_r5_sensor", 2, True)])
def test_device_set_matches_golden(tritd, orc, name, P, serial, monkeypatch):
    """tritd_set_devices: one GPU repeated P times.  Default:
    one host thread per shard steps a Session with a communicator through the
    fused two-all-reduce schedule bench.py runs (api.cpp run_group; in-process
    all-reduce for a repeated device).  TRITD_SHOV=0: the phase-serial order
    driven from the calling thread (run_group_serial)."""
    if serial:
        monkeypatch.setenv("TRITD_SHOV", "0")
    g = load_golden(name)
    tritd.set_devices([0] * P)
    try:
        got = tritd.triple_decomp_ADMM(g["D"], g["r"], g["opts"], g["A0"], g["B0"], g["C0"],
                                       return_E=True, return_iters=True)
    finally:
        tritd.set_devices([])
    check_solution(orc, got, g, g["k"])


def test_device_set_f32_and_errors(tritd, orc):
    """The fp32 path over a device set matches its single-device run; a set
    naming an absent device, or mixing repeats with other devices, fails
    like the reference's argument errors (nothing runs)."""
    from tritd import synth
    d = synth.low_rank_plus_outliers(40, 24, 36, 3, seed=5, init_seed=9)
    D = d["D"].astype(np.float32)
    opts = dict(synth.TRAFFIC_OPTS, maxIter=25)
    one = tritd.triple_decomp_ADMM(D, 3, opts, d["A0"], d["B0"], d["C0"], return_E=True,
                                   return_iters=True)
    tritd.set_devices([0, 0])
    try:
        two = tritd.triple_decomp_ADMM(D, 3, opts, d["A0"], d["B0"], d["C0"], return_E=True,
                                       return_iters=True)
    finally:
        tritd.set_devices([])
    assert one[6] == two[6] and two[3].dtype == np.float32
    assert rel(orc.triple_product(*two[:3]), orc.triple_product(*one[:3])) <= 1e-5
    assert rel(two[3].astype(np.float64), one[3].astype(np.float64)) <= 1e-5
    n = tritd.device_count()
    with pytest.raises(tritd.TritdError):
        tritd.set_devices([n])
    if n >= 2:
        tritd.set_devices([0, 0, 1])
        try:
            with pytest.raises(tritd.TritdError, match="distinct devices or one device repeated"):
                tritd.triple_decomp_ADMM(D, 3, opts, d["A0"], d["B0"], d["C0"])
        finally:
            tritd.set_devices([])


def _active_lambda(D):
    """lambda = 2e-3 std(D): with TRAFFIC_OPTS' mu = 1e-3 the soft threshold
    starts at 2 std(D) instead of 1800, so E is nonzero from the first
    iterations (with lambda = 1.8 it is identically zero over the few
    iterations of the cases below, and every comparison of E is 0 == 0)."""
    return 2e-3 * float(np.std(D))


def _medium(tritd, orc, e_active):
    from tritd import synth
    d = synth.low_rank_plus_outliers(70, 33, 50, 8, seed=3)
    opts = dict(synth.TRAFFIC_OPTS, maxIter=6)
    if e_active:
        opts["lambda"] = _active_lambda(d["D"])
    ref = orc.triple_decomp_ADMM(d["D"], 8, opts, d["A0"], d["B0"], d["C0"])
    if e_active:
        assert np.count_nonzero(ref[5]) >= 0.20 * ref[5].size
    got = tritd.triple_decomp_ADMM(d["D"], 8, opts, d["A0"], d["B0"], d["C0"], return_E=True,
                                   return_iters=True)
    A, B, C, O, eh, E, k = got
    assert k == ref[6]
    assert rel(O, ref[3]) <= TOL_LOE
    assert rel(E, ref[5]) <= TOL_LOE
    np.testing.assert_allclose(eh, ref[4], rtol=TOL_ERR, atol=ATOL_ERR)


def test_medium_against_oracle(tritd, orc):
    """A size with several workgroups per kernel and ragged padding."""
    _medium(tritd, orc, False)


def test_medium_against_oracle_e_active(tritd, orc):
    """The same with E active (nnz(E) >= 20 % in the reference)."""
    _medium(tritd, orc, True)


DEGENERATE = [((12, 10), 2), ((5, 1, 7), 2), ((1, 9, 8), 2), ((33, 17, 1), 3), ((16, 16, 16), 1)]


def _degenerate(tritd, orc, shape, r, e_active):
    rng = np.random.default_rng(11)
    D = np.asfortranarray(rng.standard_normal(shape) * 3.0)
    n1, n2, n3 = (tuple(shape) + (1,))[:3]
    A0 = rng.standard_normal((n1, r, r))
    B0 = rng.standard_normal((r, n2, r))
    C0 = rng.standard_normal((r, r, n3))
    from tritd import synth
    opts = dict(synth.TRAFFIC_OPTS, maxIter=8)
    if e_active:
        opts["lambda"] = _active_lambda(D)
    ref = orc.triple_decomp_ADMM(D, r, opts, A0, B0, C0)
    if e_active:
        assert np.count_nonzero(ref[5]) >= 0.20 * ref[5].size
    A, B, C, O, eh, E, k = tritd.triple_decomp_ADMM(D, r, opts, A0, B0, C0, return_E=True,
                                                    return_iters=True)
    assert k == ref[6]
    assert rel(orc.triple_product(A, B, C), orc.triple_product(ref[0], ref[1], ref[2])) <= 1e-8
    assert rel(O, ref[3]) <= 1e-8
    assert rel(E, ref[5]) <= 1e-8
    np.testing.assert_allclose(eh, ref[4], rtol=1e-7, atol=1e-11)


@pytest.mark.parametrize("shape,r", DEGENERATE)
def test_degenerate_shapes_against_oracle(tritd, orc, shape, r):
    """2-D D (n3 = 1 by MATLAB's trailing-singleton rule), singleton modes and r = 1:
    ragged single tiles in every padded dimension."""
    _degenerate(tritd, orc, shape, r, False)


@pytest.mark.parametrize("shape,r", DEGENERATE)
def test_degenerate_shapes_against_oracle_e_active(tritd, orc, shape, r):
    """The same shapes with E active (nnz(E) >= 20 % in the reference): the
    soft threshold and both E storage forms on singleton and ragged modes."""
    _degenerate(tritd, orc, shape, r, True)


def test_disp_prints_like_reference(tritd, orc):
    g = load_golden("g30_r3")
    opts = dict(g["opts"], disp=1, maxIter=20)
    lines = []
    tritd.set_printer(lines.append)
    try:
        tritd.triple_decomp_ADMM(g["D"], g["r"], opts, g["A0"], g["B0"], g["C0"])
    finally:
        tritd.set_printer(None)
    ref_lines = []
    orc.triple_decomp_ADMM(g["D"], g["r"], opts, g["A0"], g["B0"], g["C0"], printer=ref_lines.append)
    assert [l.split(",")[0] for l in lines] == [l.split(",")[0] for l in ref_lines] == ["Iter 10", "Iter 20"]
    assert lines == ref_lines


def test_maxiter_zero_returns_initial_factors(tritd):
    g = load_golden("g12x10x8_r2")
    A, B, C, O, eh = tritd.triple_decomp_ADMM(g["D"], g["r"], dict(g["opts"], maxIter=0),
                                              g["A0"], g["B0"], g["C0"])
    assert eh.size == 0
    np.testing.assert_array_equal(A, g["A0"])
    np.testing.assert_array_equal(B, g["B0"])
    np.testing.assert_array_equal(C, g["C0"])
    assert not O.any()


# ---------------------------------------------------------------------------
# primitives
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 10, 8), (30, 30, 30), (65, 3, 130), (1, 7, 1), (128, 64, 2),
                                   (128, 64, 128), (64, 256, 256)])  # last two: k_transpose_tall
def test_unfold_bit_exact(tritd, orc, shape):
    X = np.asfortranarray(np.random.default_rng(1).standard_normal(shape))
    for mode in (1, 2, 3):
        np.testing.assert_array_equal(tritd.unfold(X, mode), orc.unfold(X, mode))


def test_unfold_bad_mode(tritd):
    with pytest.raises(tritd.TritdError, match="Mode must be 1, 2, or 3."):
        tritd.unfold(np.zeros((2, 2, 2)), 0)


def test_soft_threshold_bit_exact(tritd, orc):
    rng = np.random.default_rng(2)
    X = rng.standard_normal(10001) * 3
    X[:6] = [0.0, -0.0, np.nan, np.inf, -np.inf, 1.8]
    for lam in (0.0, 1.8, 1e-4):
        got = tritd.soft_threshold(X, lam)
        np.testing.assert_array_equal(got, orc.soft_threshold(X, lam))
    # several grid steps of the 8-pair-per-thread kernel, a ragged tail and n odd
    for n in (2 * 8 * 256 * 3 + 7, 1 << 22):
        Y = rng.standard_normal(n)
        np.testing.assert_array_equal(tritd.soft_threshold(Y, 0.7), orc.soft_threshold(Y, 0.7))


# r = 12 and 16 (R = 144 / 256, the padded-rank 256 kernel config 5's
# reconstruction runs, traffic_triple_comparison.m:62) beside the r <= 8 forms
@pytest.mark.parametrize("n1,n2,n3,r", [(12, 10, 8, 2), (30, 31, 29, 3), (17, 16, 20, 8), (5, 4, 33, 5),
                                        (40, 36, 30, 12), (33, 20, 48, 16), (64, 64, 32, 16),
                                        # every other rank <= 16 at the ragged shapes of
                                        # tests/sweep_cases.py (r = 6: padded rank 48)
                                        (36, 23, 33, 4), (35, 20, 35, 6), (36, 21, 36, 7),
                                        (35, 23, 34, 9), (36, 19, 35, 10), (37, 20, 36, 11),
                                        (36, 22, 34, 13), (37, 23, 35, 14), (35, 19, 36, 15)])
def test_triple_product(tritd, orc, n1, n2, n3, r):
    from tritd import synth
    A, B, C = synth.random_factors(n1, n2, n3, r, seed=n1)
    got = tritd.triple_product(A, B, C)
    ref = orc.triple_product_loops(A, B, C) if n1 * n2 * n3 * r * r < 200000 else orc.triple_product(A, B, C)
    assert rel(got, ref) <= 1e-13


@pytest.mark.parametrize("r", [2, 3, 5])
def test_design_matrices_bit_exact(tritd, orc, r):
    from tritd import synth
    A, B, C = synth.random_factors(9, 7, 6, r, seed=r)
    np.testing.assert_array_equal(tritd.buildF(B, C), orc.buildF(B, C))
    np.testing.assert_array_equal(tritd.buildG(A, C), orc.buildG(A, C))
    np.testing.assert_array_equal(tritd.buildH(A, B), orc.buildH(A, B))


# The wide-rank goldens (g20x18x16_r10, g24x20x18_r12, g24x22x20_r16) stop while the
# threshold lambda/mu is still above every entry: their E is identically zero,
# so this test pins the factors, L and O at r = 9..16 but not the outlier
# chain.  tests/test_gpu_rank_sweep.py covers those ranks with E active.
@pytest.mark.parametrize("name", ["g20x18x16_r10", "g24x22x20_r16"])
def test_fp64_session_wide_rank_matches_golden(tritd, orc, name):
    """fp64 sessions (the bench / one-process-per-GPU path) take r = 9..16 like
    the one-shot solver."""
    g = load_golden(name)
    n1, n2, n3 = g["D"].shape
    s = tritd.Session(g["r"], g["opts"], g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3,
                      D=g["D"], device=0)
    s.run(g["opts"]["maxIter"])
    r = s.get()
    s.close()
    check_solution(orc, (r["A"], r["B"], r["C"], r["O"], r["errHist"], r["E"], r["k"]), g, g["k"])


def _near_tol_case(orc):
    """A stop test that fires within 1e-7 (relative) of opts.tol: tol is set just
    above the relative change rho_m = |e_m - e_(m-1)| / e_(m-1) of an iteration
    m whose rho is a strict running minimum (:63), so the reference stops at m;
    just below it, it does not.  The GPU's errHist agrees to ~1e-12, so its
    rho agrees to ~1e-10 relative: both tols must give the reference's k.
    (K5 accumulates the residual norms with FMAs in its own order, DESIGN.md
    §2; this pins the stop decision under that default.)"""
    from tritd import synth
    d = synth.low_rank_plus_outliers(24, 20, 18, 3, seed=21, init_seed=4)
    opts = dict(synth.TRAFFIC_OPTS, maxIter=40, tol=0.0)
    *_, eh, _, k, _ = orc.triple_decomp_ADMM(d["D"], 3, opts, d["A0"], d["B0"], d["C0"])
    assert k == 40
    rho = np.abs(np.diff(eh)) / eh[:-1]  # rho[m-2] belongs to iteration m
    for m in range(6, 41):
        if rho[m - 2] * (1 + 1e-6) < rho[: m - 2].min():
            break
    else:
        pytest.skip("no strict running minimum of the relative change")
    return d, opts, m, rho[m - 2]


@pytest.mark.parametrize("schedule", ["one_gpu", "rccl_one_rank"])
def test_stop_iteration_near_tolerance(tritd, orc, schedule):
    d, opts, m, rho = _near_tol_case(orc)
    n1, n2, n3 = d["D"].shape
    for tol in (rho * (1 + 1e-7), rho * (1 - 1e-7)):
        o = dict(opts, tol=float(tol))
        ref = orc.triple_decomp_ADMM(d["D"], 3, o, d["A0"], d["B0"], d["C0"])
        comm = tritd.Comm(tritd.Comm.unique_id(), 1, 0, 0) if schedule == "rccl_one_rank" else None
        s = tritd.Session(3, o, d["A0"], d["B0"], d["C0"], n1=n1, n2=n2, n3=n3, D=d["D"], device=0,
                          comm=comm)
        s.run(o["maxIter"])
        res = s.get()
        s.close()
        if comm is not None:
            comm.close()
        assert res["k"] == ref[6]
        assert (ref[6] == m) == (tol > rho)
        got = (res["A"], res["B"], res["C"], res["O"], res["errHist"], res["E"], res["k"])
        check_solution(orc, got, dict(A=ref[0], B=ref[1], C=ref[2], O=ref[3], errHist=ref[4],
                                      E=ref[5]), ref[6])
