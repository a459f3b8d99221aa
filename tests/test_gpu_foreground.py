"""Foreground detection on the GPU (eval of
video_triple_comparison.m:316-371): the mask abs(O) > thr and the per-frame
TP / FP / FN / TN, taken from a session's resident D, Y_L and T without O ever
being rebuilt, against tests/foreground_oracle.py.  Inputs:
tests/foreground_cases.py, admitted on the CPU by tests/test_foreground_cases.py.
Masks and counts are integers: every comparison here is exact.

1. The primitives (tritd.foreground_eval, tritd_dev_foreground_*) equal the
   oracle on the cases' O in float64 and float32, on a tensor of special
   values (NaN, +-Inf, -0.0, +-thr, its neighbours, thr = 0), on planes that
   take the 16-byte path and the byte path, with leading dimensions.
2. ADMM sessions (fp64 r = 5 and 11, fp32 r = 5 and 16, masked, holdout):
   before the first iteration the mask is all false; after 3 and after 3 + 7
   iterations mask == (abs(get()["O"]) > thr) and counts == eval_counts of that
   O; a masked session predicts nothing at an unobserved entry; a twin session
   that never called foreground returns bitwise the same get().
3. The fp64 forms give the mask and counts of the oracle's O (the admission
   gap of the cases against the suite's O tolerances).
4. A shard [5, n1 - 4) with gt inside the whole ground truth (ldG = n1) and
   pred with ldP = nl + 3: the standalone result in rows < nl, every other
   byte untouched; the device form is bitwise the host form; three ranks on
   one GPU (host transport) give counts that add up to the one-session counts.
5. The nonconvex AlsSession: mask == (abs(get_O()) > thr) and exact counts
   on a run to maxIter and on one stopped by tol (O of k - 1); TRITD_ERR_STATE
   on a plain ALS session.
6. drivers.video_triple(X, groundtruth=G) prints the five lines of :366-370
   with the oracle's numbers on the O it returns.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import foreground_cases as fc
import foreground_oracle as fo
import sweep_cases as sc
from conftest import load_golden

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 8
THR = fc.THR
MASKED_CASE = "sweep36_r5"
FORMS = list(fc.CASES) + ["masked", "holdout"]
FORMS64 = list(fc.F64_CASES) + ["masked"]


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def hip(tritd):
    from tritd import hip as h
    return h


def expect(F, G, thr=THR):
    counts = fo.eval_counts(F, G, thr)
    return fo.pred_mask(F, thr), counts, fo.scores(counts, np.asarray(F).size)


def same_scores(got, want):
    assert (got["total"] == want["total"]).all()
    for k in ("precision", "recall", "f1", "pwc"):
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), k


def check_result(res, F, G, thr=THR):
    mask, counts, s = expect(F, G, thr)
    assert res["mask"].dtype == np.bool_ and res["mask"].shape == np.asarray(F).shape
    assert (res["mask"] == mask).all(), np.argwhere(res["mask"] != mask)[:5]
    assert res["counts"].dtype == np.int64 and (res["counts"] == counts).all()
    same_scores(res, s)


# --- 1. primitives --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_primitive_equals_the_oracle_on_the_cases(tritd, name):
    O, G = fc.oracle_O(name), fc.case(name)["G"]
    check_result(tritd.foreground_eval(O, G, THR), O, G)
    O32 = np.asfortranarray(O, dtype=np.float32)
    check_result(tritd.foreground_eval(O32, G, THR), O32, G)
    only_mask = tritd.foreground_eval(O)  # the reference's thr, no ground truth
    assert set(only_mask) == {"mask"} and (only_mask["mask"] == fo.pred_mask(O, 50.0)).all()


@pytest.mark.parametrize("thr", [THR, 0.0])
def test_primitive_special_values(tritd, thr):
    F, G = fc.special_values(thr if thr else THR)
    with np.errstate(over="ignore"):  # 1e308 as single is Inf, on purpose
        F32 = np.asfortranarray(F, dtype=np.float32)
    for X in (F, F32):
        check_result(tritd.foreground_eval(X, G, thr), X, G, thr)
    # a threshold that single cannot hold: the comparison is made in double
    t = float(np.nextafter(np.float32(THR), np.float32(np.inf))) - 1e-9
    check_result(tritd.foreground_eval(F32, G, t), F32, G, t)


@pytest.mark.parametrize("shape", [(64, 80, 3), (37, 113, 2), (5, 1, 1), (1, 1, 40), (16, 1024, 2)])
def test_primitive_planes_of_every_path(tritd, shape):
    """n1 n2 a multiple of 16 or not, one chunk of 4096 or several, trailing dims folded"""
    rng = np.random.default_rng(sum(shape))
    F = np.asfortranarray(rng.normal(0, 60, size=shape))
    G = np.asfortranarray(rng.choice(np.array(fc.LABELS, dtype=np.uint8), size=shape))
    check_result(tritd.foreground_eval(F, G, THR), F, G)
    F4 = F.reshape(shape[:2] + (1, shape[2]), order="F")
    res = tritd.foreground_eval(F4, G.reshape(F4.shape, order="F"), THR)
    assert res["mask"].shape == F4.shape and (res["counts"] == fo.eval_counts(F, G, THR)).all()


@pytest.mark.parametrize("f32", [False, True])
def test_device_primitive_with_leading_dimensions(tritd, hip, f32):
    from tritd import _lib
    n1, n2, nf = 21, 7, 5
    rng = np.random.default_rng(8)
    dt = np.float32 if f32 else np.float64
    F = np.asfortranarray(rng.normal(0, 60, size=(n1, n2, nf)).astype(dt))
    G = np.asfortranarray(rng.choice(np.array(fc.LABELS, dtype=np.uint8), size=F.shape))
    ldF, ldG, ldP = n1 + 3, n1 + 1, n1 + 2
    Fp = np.full((ldF, n2, nf), np.nan, dtype=dt, order="F")
    Fp[:n1] = F
    Gp = np.full((ldG, n2, nf), 255, dtype=np.uint8, order="F")
    Gp[:n1] = G
    Pp = np.full((ldP, n2, nf), 0xAB, dtype=np.uint8, order="F")
    dF, dG, dP = (hip.DeviceArray.from_host(a) for a in (Fp, Gp, Pp))
    counts = np.zeros((nf, 4), dtype=np.int64)
    fn = _lib.lib.tritd_dev_foreground_f32 if f32 else _lib.lib.tritd_dev_foreground_f64
    try:
        _lib.check(fn(dF.ptr, ldF, dG.ptr, ldG, n1, n2, nf, THR, dP.ptr, ldP,
                      C.c_void_p(counts.ctypes.data), None))
        dP.to_host(Pp)
    finally:
        for d in (dF, dG, dP):
            d.free()
    mask, want, _ = expect(F, G)
    assert (Pp[:n1].view(np.bool_) == mask).all() and (Pp[n1:] == 0xAB).all()
    assert (counts == want).all()


# --- 2. / 3. ADMM sessions ---------------------------------------------------------------
def open_session(tritd, form, **kw):
    name = MASKED_CASE if form in ("masked", "holdout") else form
    c = fc.case(name)
    n1, n2, n3 = c["shape"]
    if form in ("masked", "holdout"):
        kw["observed"] = fc.observed_mask(name)
    if form == "holdout":
        kw["holdout"] = fc.holdout_mask(name)
    return tritd.Session(c["r"], c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                         D=c["D"], probe=False, device=0, **kw), c


@functools.lru_cache(maxsize=None)
def session_run(form):
    """One session that calls foreground before the first iteration, after 3
    and after 3 + 7, and a twin that never does: -> dict(fg0, fg3, fg10, get3,
    get10, twin3, twin10, G).  Computed once per form and shared."""
    import tritd
    s, c = open_session(tritd, form)
    t, _ = open_session(tritd, form)
    G = c["G"]
    try:
        out = dict(G=G, fg0=s.foreground(THR, G))
        for s_, keys in ((s, ("fg", "get")), (t, (None, "twin"))):
            for iters, tag in ((3, "3"), (fc.ITERS - 3, "10")):
                s_.run(iters)
                if keys[0]:
                    out[keys[0] + tag] = s_.foreground(THR, G)
                out[keys[1] + tag] = s_.get()
    finally:
        s.close()
        t.close()
    return out


@pytest.mark.parametrize("form", FORMS)
def test_session_mask_is_that_of_get_bitwise(tritd, form):
    r = session_run(form)
    G = r["G"]
    zero = np.zeros(G.shape)
    check_result(r["fg0"], zero, G)  # before any iteration O is 0
    assert not r["fg0"]["mask"].any()
    for tag in ("3", "10"):
        O = r["get" + tag]["O"]
        assert r["get" + tag]["k"] == int(tag)
        check_result(r["fg" + tag], O, G)
        assert r["fg" + tag]["mask"].any() and not r["fg" + tag]["mask"].all()
    if form in ("masked", "holdout"):
        obs = fc.observed_mask(MASKED_CASE)
        assert not r["fg3"]["mask"][~obs].any() and not r["fg10"]["mask"][~obs].any()


@pytest.mark.parametrize("form", FORMS)
def test_foreground_leaves_the_iterates_untouched(tritd, form):
    r = session_run(form)
    for tag in ("3", "10"):
        a, b = r["get" + tag], r["twin" + tag]
        assert a["k"] == b["k"]
        for key in ("A", "B", "C", "O", "E", "errHist"):
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape
            assert a[key].tobytes(order="A") == b[key].tobytes(order="A"), (tag, key)


@pytest.mark.parametrize("form", FORMS64)
def test_session_mask_is_that_of_the_oracle(tritd, form):
    r = session_run(form)
    for iters, tag in ((3, "3"), (fc.ITERS, "10")):
        O = fc.oracle_O_masked(MASKED_CASE, iters) if form == "masked" else fc.oracle_O(form, iters)
        check_result(r["fg" + tag], O, r["G"])


def test_session_python_forms_and_argument_rules(tritd, hip):
    from tritd import _lib
    s, c = open_session(tritd, "pad21_r5")
    G = c["G"]
    nl, n2, n3 = G.shape
    try:
        s.run(4)
        full = s.foreground(THR, G)
        assert set(full) == {"mask", "counts", "total", "precision", "recall", "f1", "pwc"}
        assert set(s.foreground(THR)) == {"mask"}
        no_mask = s.foreground(THR, G, return_mask=False)
        assert "mask" not in no_mask and (no_mask["counts"] == full["counts"]).all()
        # labels given as doubles: the same two values count
        assert (s.foreground(THR, G.astype(np.float64))["counts"] == full["counts"]).all()
        other = s.foreground(0.5 * THR, G)
        check_result(other, s.get()["O"], G, 0.5 * THR)
        assert other["mask"].sum() > full["mask"].sum()
        # the rules, in their order, on a live session; nothing is written
        P = np.full(G.shape, 0xAB, dtype=np.uint8, order="F")
        cnt = np.full((n3, 4), -7, dtype=np.int64)
        p = lambda a: C.c_void_p(a.ctypes.data)
        fn = _lib.lib.tritd_session_foreground
        for args, msg in (((-1.0, p(G), nl, p(P), nl, p(cnt), 0), "thr must be >= 0"),
                          ((float("nan"), p(G), nl, p(P), nl, p(cnt), 0), "thr must be >= 0"),
                          ((-1.0, None, nl, None, nl, p(cnt), 0), "thr must be >= 0"),
                          ((THR, None, nl, None, nl, p(cnt), 0), "both NULL"),
                          ((THR, p(G), nl, p(P), nl, None, 0), "counts is NULL"),
                          ((THR, p(G), nl - 1, p(P), nl, p(cnt), 0), "ldG smaller than the shard"),
                          ((THR, p(G), nl, p(P), nl - 1, p(cnt), 0), "ldP smaller than the shard"),
                          ((THR, None, nl - 1, p(P), nl - 1, None, 0), "ldP smaller than the shard")):
            assert fn(s._s, *args) == ARG, args
            assert msg in _lib.lib.tritd_last_error().decode(), (args, msg)
        assert (P == 0xAB).all() and (cnt == -7).all()
        # a mask alone needs no counts; a NULL gt's leading dimension is not looked at
        _lib.check(fn(s._s, THR, None, 0, p(P), nl, None, 0))
        assert (P.view(np.bool_) == full["mask"]).all()
        again = s.foreground(THR, G)
        assert (again["mask"] == full["mask"]).all() and (again["counts"] == full["counts"]).all()
    finally:
        s.close()


# --- 4. shards and leading dimensions ---------------------------------------------------
def test_shard_with_leading_dimensions_and_device_form(tritd, hip):
    from tritd import _lib
    c = fc.case("sweep36_r5")
    n1, n2, n3 = c["shape"]
    i0, i1 = 5, n1 - 4
    nl = i1 - i0
    G = c["G"]
    Ds = np.asfortranarray(c["D"][i0:i1])
    alone = tritd.Session(c["r"], c["opts"], np.asfortranarray(c["A0"][i0:i1]), c["B0"], c["C0"],
                          n1=nl, n2=n2, n3=n3, D=Ds, probe=False, device=0)
    shard = tritd.Session(c["r"], c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                          i0=i0, i1=i1, D=Ds, probe=False, device=0)
    try:
        alone.run(fc.ITERS)
        shard.run(fc.ITERS)
        want = alone.foreground(THR, np.asfortranarray(G[i0:i1]))
        check_result(want, alone.get()["O"], G[i0:i1])
        assert want["mask"].any()
        # gt inside the whole ground truth, pred with three spare rows per fibre
        ldP = nl + 3
        P = np.full((ldP, n2, n3), 0xAB, dtype=np.uint8, order="F")
        cnt = np.zeros((n3, 4), dtype=np.int64)
        _lib.check(_lib.lib.tritd_session_foreground(
            shard._s, THR, C.c_void_p(G.ctypes.data + i0), n1, C.c_void_p(P.ctypes.data), ldP,
            C.c_void_p(cnt.ctypes.data), 0))
        assert (P[:nl].view(np.bool_) == want["mask"]).all() and (P[nl:] == 0xAB).all()
        assert (cnt == want["counts"]).all()
        # the Python form on a view of the whole ground truth (its strides give ldG = n1)
        view = shard.foreground(THR, G[i0:i1])
        assert (view["mask"] == want["mask"]).all() and (view["counts"] == want["counts"]).all()
        # device form: gt (ldG = n1, offset i0) and pred (ldP = nl + 3) in device memory
        dG = hip.DeviceArray.from_host(G)
        dP = hip.DeviceArray.from_host(np.full((ldP, n2, n3), 0xAB, dtype=np.uint8, order="F"))
        try:
            dev = shard.foreground(THR, gt_device_ptr=dG.ptr + i0, ldG=n1, mask_device_ptr=dP.ptr,
                                   ldP=ldP)
            Pd = dP.to_host(np.zeros((ldP, n2, n3), dtype=np.uint8, order="F"))
        finally:
            dG.free()
            dP.free()
        assert "mask" not in dev and (dev["counts"] == want["counts"]).all()
        assert np.array_equal(Pd, P)
    finally:
        alone.close()
        shard.close()


class ThreadRanks:
    """A host transport for `world` ranks that are threads of this process:
    every rank adds (or maximises) the ranks' buffers in rank order."""

    def __init__(self, world):
        self.world, self.slots = world, [None] * world
        self.bar = threading.Barrier(world, timeout=60)

    def reducer(self, rank):
        def fn(buf, op):
            self.slots[rank] = buf.copy()
            self.bar.wait()
            out = self.slots[0].copy()
            for q in range(1, self.world):
                out = np.maximum(out, self.slots[q]) if op else out + self.slots[q]
            self.bar.wait()
            buf[:] = out
        return fn


def test_three_ranks_on_one_gpu_add_up_to_the_one_session_counts(tritd):
    from tritd.dist import all_bounds
    name = "sweep36_r5"
    c = fc.case(name)
    n1, n2, n3 = c["shape"]
    G = c["G"]
    world = 3
    ranks, out, errs = ThreadRanks(world), [None] * world, []

    def work(rank, i0, i1):
        try:
            comm = tritd.Comm.host(ranks.reducer(rank), world, rank, 0)
            try:
                s = tritd.Session(c["r"], c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                                  i0=i0, i1=i1, D=np.asfortranarray(c["D"][i0:i1]), probe=False,
                                  device=0, comm=comm)
                try:
                    s.run(fc.ITERS)
                    out[rank] = s.foreground(THR, G[i0:i1])
                finally:
                    s.close()
            finally:
                comm.close()
        except BaseException as e:  # reported by the main thread
            errs.append(e)
            ranks.bar.abort()

    ts = [threading.Thread(target=work, args=(q, *b)) for q, b in enumerate(all_bounds(n1, world))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs
    assert not any(t.is_alive() for t in ts)
    one = session_run(name)["fg10"]
    assert (sum(r["counts"] for r in out) == one["counts"]).all()
    assert (np.concatenate([r["mask"] for r in out], axis=0) == one["mask"]).all()
    # a rank's scores are those of its rows alone: nothing is reduced across ranks
    for r, (i0, i1) in zip(out, all_bounds(n1, world)):
        same_scores(r, fo.scores(r["counts"], (i1 - i0) * n2 * n3))


# --- 5. the nonconvex AlsSession -----------------------------------------------------------
def ncvx_session(tritd, X, r, A0, B0, C0, prm):
    n1, n2, n3 = X.shape
    return tritd.AlsSession(r, dict(maxIter=prm["maxIter"], tol=prm["tol"]), A0, B0, C0, n1=n1, n2=n2,
                            n3=n3, X=X, device=0,
                            ncvx={k: prm[k] for k in ("rho", "lam", "gamma_A", "epsilon", "p", "theta")})


def test_ncvx_session_to_maxiter(tritd):
    c = fc.case("pad21_r5")
    s = ncvx_session(tritd, c["D"], c["r"], c["A0"], c["B0"], c["C0"], sc.NCVX_PARAMS)
    try:
        check_result(s.foreground(THR, c["G"]), np.zeros(c["shape"]), c["G"])  # the zero initial O
        s.run(3)
        check_result(s.foreground(THR, c["G"]), s.get_O(), c["G"])
        s.run(sc.NCVX_PARAMS["maxIter"])
        assert s.sync() == (sc.NCVX_PARAMS["maxIter"], False)
        O = s.get_O()
        res = s.foreground(THR, c["G"])
        check_result(res, O, c["G"])
        assert res["mask"].any() and not res["mask"].all()
        assert np.array_equal(s.get_O(), O)
    finally:
        s.close()


def test_ncvx_session_stopped_by_tol_uses_the_previous_O(tritd):
    g = load_golden("nc20x24x18_r3_stop")
    o = g["opts"]
    prm = dict(o, lam=o["lambda"])
    G = np.asfortranarray(np.random.default_rng(4).choice(np.array(fc.LABELS, dtype=np.uint8),
                                                           size=g["X"].shape))
    s = ncvx_session(tritd, g["X"], g["r"], g["A0"], g["B0"], g["C0"], prm)
    try:
        s.run(o["maxIter"])
        assert s.sync() == (g["k"], True)
        O = s.get_O()
        res = s.foreground(THR, G)
        check_result(res, O, G)
        assert res["mask"].any() and not res["mask"].all()
    finally:
        s.close()


def test_plain_als_session_is_a_state_error(tritd):
    c = fc.case("full16_r5")
    n1, n2, n3 = c["shape"]
    s = tritd.AlsSession(c["r"], sc.ALS_OPTS, c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3,
                         X=c["D"], device=0)
    try:
        s.run(2)
        with pytest.raises(tritd.TritdError) as e:
            s.foreground(THR, c["G"])
        assert e.value.status == STATE and "not a nonconvex" in str(e.value)
    finally:
        s.close()


# --- 6. the video driver --------------------------------------------------------------------
def test_video_driver_prints_the_five_lines(tritd):
    from tritd import drivers
    c = fc.case("pad21_r5")
    lines = []
    out = drivers.video_triple(c["D"], r=c["r"], opts=dict(c["opts"], disp=0), A0=c["A0"], B0=c["B0"],
                               C0=c["C0"], printer=lines.append, groundtruth=c["G"])
    mask, counts, s = expect(out["O"], c["G"], 50.0)
    assert len(lines) == 7 and lines[1].startswith("TRIPLE ADMM - RMSE:")
    assert lines[2:] == fo.report_lines(s)
    assert (out["fg_mask"] == mask).all() and (out["fg_counts"] == counts).all()
    for k in ("precision", "recall", "f1", "pwc"):
        assert out[k] == s[k]
    assert mask.any()
    # another threshold goes through
    out2 = drivers.video_triple(c["D"], r=c["r"], opts=dict(c["opts"], disp=0), A0=c["A0"],
                                B0=c["B0"], C0=c["C0"], printer=lambda s_: None, groundtruth=c["G"],
                                thr=20.0)
    assert (out2["fg_mask"] == fo.pred_mask(out2["O"], 20.0)).all()
