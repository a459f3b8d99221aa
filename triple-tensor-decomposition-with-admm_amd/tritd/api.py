"""Reference-mirroring host API (the MATLAB call surface, in Python).

Every function here keeps the name, argument meaning and failure behaviour of
the MATLAB file it replaces and runs on the GPU through libtritd.so:

    triple_decomp_ADMM(D, r, opts)          fast_robust_triple_tensor/triple_decomp_ADMM.m:1
    triple_decomp_ADMM_outlier(D, r, opts)  alias expected at video_triple_comparison.m:54
    triple_decomp_ADMM_outlier(X, r, rho, lambda, gamma_A, epsilon, p, theta, maxIter, tol)
                                            fast_robust_triple_tensor/test.m:1 (nonconvex variant)
    triple_decomp_ALS(X, r, opts)           fast_robust_triple_tensor/triple_decomp_ALS.m:1
    triple_product(A, B, C[, model])        triple_product.m:1 (model='qi': origin_triple_tensor/)
    unfold(X, mode)                         unfold.m:1
    soft_threshold(X, lam)                  soft_threshold.m:1
    buildF(B, C) / buildG(A, C) / buildH(A, B)   buildF.m:1 / buildG.m:1 / buildH.m:1
    evaluate(X, gt, mask)                   traffic_triple_comparison.m:194-202
    foreground_eval(F, groundtruth, thr)    video_triple_comparison.m:316-371 (eval)
    quality_ybz(X1, X2)                     other_methods/Low-rank-.../quality_ybz.m:1

Arrays are numpy, MATLAB (column-major) semantics.  `opts` is a dict (or any
object with attributes) holding the fields the reference reads
(mu, rho, lambda, lambda2, maxIter, tol, disp); a missing one raises
``KeyError("Reference to non-existent field 'x'.")`` like MATLAB, extras
(alphaA, alphaB, origin, ...) are ignored.  One optional field is this
build's own: ``opts.model`` = 'cp' (default: the executed rank-r^2 CP builders)
or 'qi' (Qi's 3-index triple product, origin_triple_tensor/build{F,G,H}.m;
SURVEY.md §8f rank 4).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PinvToleranceWarning, TritdError, check, check_flags, lib

REQUIRED = ("mu", "rho", "lambda", "lambda2", "maxIter", "tol", "disp")


def _get(opts, name):
    if isinstance(opts, dict):
        return opts[name] if name in opts else None
    return getattr(opts, name, None)


def make_opts(opts):
    """dict/struct -> tritd_opts; raises like MATLAB on a missing field."""
    o = _lib.Opts()
    present = 0
    for name in REQUIRED:
        v = _get(opts, name)
        if v is None:
            raise KeyError(f"Reference to non-existent field '{name}'.")
        present |= _lib.OPT_BITS[name]
    o.mu = float(_get(opts, "mu"))
    o.rho = float(_get(opts, "rho"))
    o.lambda_ = float(_get(opts, "lambda"))
    o.lambda2 = float(_get(opts, "lambda2"))
    o.tol = float(_get(opts, "tol"))
    o.maxIter = int(_get(opts, "maxIter"))
    o.disp = int(bool(_get(opts, "disp")))
    o.present = present
    o.model = model_code(_get(opts, "model"))
    return o


def model_code(m):
    """opts.model -> TRITD_MODEL_*: absent/'cp' -> 0, 'qi' -> 1."""
    if m is None:
        return 0
    key = str(m).lower()
    if key not in _lib.MODELS:
        raise ValueError("opts.model must be 'cp' or 'qi'")
    return _lib.MODELS[key]


def _f64(X):
    return np.asarray(X, dtype=np.float64)


def _fortran(X):
    return np.asfortranarray(_f64(X))


def _size3(X):
    if X.ndim > 3:
        raise ValueError("D must have at most 3 dimensions")
    s = tuple(X.shape) + (1, 1, 1)
    return int(s[0]), int(s[1]), int(s[2])


class _ObservedNaN:
    """observed="nan": Omega = ~isnan(D), derived on the device
    (TRITD_OBSERVED_NAN of tritd.h: the constant 1 as a pointer, no array)."""

    def __repr__(self):
        return "observed='nan'"


_NAN = _ObservedNaN()


def _ptr(a):
    if a is _NAN:
        return C.c_void_p(1)
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _check_observed(observed):
    """A string ``observed`` must be exactly "nan" (NaN in the data marks a
    missing entry); any other string is a ValueError."""
    if isinstance(observed, str) and observed != "nan":
        raise ValueError(f'observed must be a logical array or the string "nan", got {observed!r}')


def _device_mask(observed):
    """``observed`` beside a device-resident tensor: a device address, "nan" or None"""
    if isinstance(observed, str):
        _check_observed(observed)
        return _ptr(_NAN)
    return C.c_void_p(int(observed)) if observed is not None else None


def _holdout_count(hold, obs, D):
    """|H & Omega| on the host; with observed="nan" from the held entries only"""
    if obs is _NAN:
        return int(np.count_nonzero(~np.isnan(D[hold.view(np.bool_)])))
    return int(np.count_nonzero(hold if obs is None else hold & obs))


def _observed_bytes(observed, shape, what="D", name="observed"):
    """opts.observed -> a column-major uint8 array of D's shape (nonzero =
    observed); a shape that differs from D's raises like a MATLAB logical
    index of the wrong size.  observed="nan" -> _NAN (no array is made)."""
    if isinstance(observed, str):
        if name != "observed":
            raise ValueError(f"{name} must be a logical array of the shape of {what}")
        _check_observed(observed)
        return _NAN
    m = np.asarray(observed)
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"{name} must have the shape of {what} {tuple(shape)}, got {tuple(m.shape)}")
    return np.asfortranarray(m != 0).view(np.uint8)


def initial_factors(n1, n2, n3, r, opts=None, rng=None):
    """A0, B0, C0 in the order of triple_decomp_ADMM.m:23.  Explicit
    opts['A0'/'B0'/'C0'] win (MATLAB's Ziggurat randn is not reproducible
    outside MATLAB, so callers that need parity pass them in)."""
    A0 = _get(opts, "A0") if opts is not None else None
    B0 = _get(opts, "B0") if opts is not None else None
    C0 = _get(opts, "C0") if opts is not None else None
    rng = rng if rng is not None else np.random.default_rng()
    if A0 is None:
        A0 = rng.standard_normal((n1, r, r))
    if B0 is None:
        B0 = rng.standard_normal((r, n2, r))
    if C0 is None:
        C0 = rng.standard_normal((r, r, n3))
    A0 = _fortran(A0).reshape((n1, r, r), order="F")
    B0 = _fortran(B0).reshape((r, n2, r), order="F")
    C0 = _fortran(C0).reshape((r, r, n3), order="F")
    return A0, B0, C0


class _OneShot:
    """One one-shot solve as the four public functions make it: the normalised
    initial factors, the output arrays (factors, ``tensors`` of the data's
    type, errHist, k, and the holdout outputs when ``hold`` is given; ``l1``:
    valHist1 too), the C call and the returned tuple."""

    def __init__(self, X, r, maxIter, opts, A0, B0, C0, *, tensors, obs=None, hold=None, l1=True):
        self.X, self.obs, self.hold = X, obs, hold
        n1, n2, n3 = _size3(X)
        self.dims = (n1, n2, n3, int(r))
        if A0 is None or B0 is None or C0 is None:
            self.start = initial_factors(*self.dims, opts)
        else:
            self.start = initial_factors(*self.dims, dict(A0=A0, B0=B0, C0=C0))
        self.factors = [np.zeros(a.shape, order="F") for a in self.start]
        # (a tensor the caller does not want back is not allocated: null to the library)
        self.tensors = [np.zeros((n1, n2, n3), order="F", dtype=X.dtype) if want else None
                        for want in tensors]
        hist = max(maxIter, 1)
        self.errHist, self.k = np.zeros(hist), _lib.i32(0)
        if hold is not None:
            self.best = [np.zeros_like(a) for a in self.factors]
            self.val = [np.zeros(hist) for _ in range(2 if l1 else 1)]
            self.best_iter, self.why = _lib.i32(0), _lib.i32(0)

    def solve(self, symbols, what, params, device, holdout_params=(), virtual_shards=0, form=None):
        """Call ``symbols[form]``; the form follows from the arguments unless given."""
        if form is None:
            form = ("holdout" if self.hold is not None else
                    "virtual" if virtual_shards and virtual_shards > 1 else
                    "masked" if self.obs is not None else "plain")
        holdout = form == "holdout"
        args = [_ptr(self.X)]
        if holdout or form == "masked":
            args.append(_ptr(self.obs))
        if holdout:
            args.append(_ptr(self.hold))
        args += [*self.dims, *params]
        if holdout:
            args += holdout_params
        args += [_ptr(a) for a in self.start]
        if form == "virtual":
            args.append(int(virtual_shards))
        args += [_ptr(a) for a in (*self.factors, *self.tensors, self.errHist)]
        args.append(C.byref(self.k))
        if holdout:
            args += [_ptr(a) for a in (*self.best, *self.val)]
            args += [C.byref(self.best_iter), C.byref(self.why)]
        check_flags(getattr(lib, symbols[form])(*args, int(device)), what)

    def result(self, leading, trailing=()):
        """(A, B, C, *leading, errHist(1:k), *trailing[, the holdout dict]);
        a ``_K`` in ``trailing`` stands for the iteration count."""
        k = self.k.value
        out = [*self.factors, *leading, self.errHist[:k].copy()]
        out += [k if t is _K else t for t in trailing]
        if self.hold is not None:
            d = dict(zip(("valHist", "valHist1"), (v[:k].copy() for v in self.val)))
            d.update(best_iter=self.best_iter.value, stop_reason=self.why.value,
                     A_best=self.best[0], B_best=self.best[1], C_best=self.best[2],
                     holdout_count=_holdout_count(self.hold, self.obs, self.X))
            out.append(d)
        return tuple(out)


_K = object()  # _OneShot.result: the iteration count goes here

_ADMM = dict(plain="tritd_admm_f64", masked="tritd_admm_masked_f64",
             holdout="tritd_admm_holdout_f64", virtual="tritd_admm_sharded_virtual_f64",
             f32="tritd_admm_f32")
_ALS = dict(plain="tritd_als_f64", masked="tritd_als_masked_f64", holdout="tritd_als_holdout_f64",
            virtual="tritd_als_sharded_virtual_f64")
_NCVX = dict(plain="tritd_ncvx_f64", masked="tritd_ncvx_masked_f64",
             holdout="tritd_ncvx_holdout_f64")


def _masks(observed, holdout, X, what, virtual_shards=0):
    """observed=, holdout= of a one-shot call -> (obs, hold) byte arrays (or None, _NAN)"""
    obs = hold = None
    if observed is not None:
        obs = _observed_bytes(observed, X.shape, what)
        if virtual_shards and virtual_shards > 1:
            raise ValueError("observed with virtual_shards: use set_devices([d] * P) and device=-1")
    if holdout is not None:
        hold = _observed_bytes(holdout, X.shape, what, "holdout")
        if virtual_shards and virtual_shards > 1:
            raise ValueError("holdout with virtual_shards: use set_devices([d] * P) and device=-1")
    return obs, hold


def triple_decomp_ADMM(D, r, opts, A0=None, B0=None, C0=None, *, device=-1, return_E=False,
                       return_iters=False, virtual_shards=0, observed=None, holdout=None,
                       patience=0, val_norm=2):
    """[A,B,C,O,errHist] = triple_decomp_ADMM(D, r, opts) on the GPU.

    ``observed`` (a logical array of D's shape, True = observed) fits the
    observed entries only (tritd_admm_masked_f64): D's values at the other
    entries are never used (NaN allowed), O and E are exactly 0 there, and
    errHist counts observed entries only.  float64 D; for mode-1 shards set
    the device set (``set_devices``), not ``virtual_shards``.

    ``observed="nan"`` (exactly that string) takes the mask from the data:
    Omega = ~isnan(D), derived on the device (TRITD_OBSERVED_NAN), with no host
    pass over D, no mask array and no upload.  Any NaN counts as missing, Inf
    is data; every output is bit for bit that of ``observed=~np.isnan(D)``.
    The other solvers and the session classes take it the same way.

    ``holdout`` (a logical array of D's shape; tritd_admm_holdout_f64) withholds
    the entries of ``holdout & observed`` from the fit, which is exactly the
    masked one with ``observed & ~holdout``, and scores them after every
    iteration k with L_k = triple_product of the factors after its updates:
    ``valHist(k) = ||H o Omega o (D - L_k)|| / ||H o Omega o D||`` and
    ``valHist1(k) = sum|D - L_k| / sum|D|`` over H & Omega (the one to read when
    the held-out entries carry outliers).  The returned tuple then gains a
    trailing dict with ``valHist``, ``valHist1``, ``best_iter`` (the first
    minimum of the history ``val_norm`` picks: 2 valHist, 1 valHist1),
    ``stop_reason`` (0 maxIter, 1 the test of :63, 2 patience), ``A_best,
    B_best, C_best`` (the factors after iteration best_iter; O and E of that
    iterate are not kept) and ``holdout_count``.  ``patience = p > 0`` stops
    the loop at k once ``k - best_iter >= p``.

    Extra outputs beyond the reference signature: E (``return_E``) and the
    iteration count (``return_iters``).  ``virtual_shards=P`` runs the mode-1
    sharded schedule as P shards on one device (rehearsal of the multi-GPU
    path).  A float32 D runs the single-class path (MATLAB semantics of a
    `single` D: O, E float32; A, B, C, errHist float64), r <= 16."""
    o = make_opts(opts)
    _check_observed(observed)
    f32 = np.asarray(D).dtype == np.float32
    if f32 and (observed is not None or holdout is not None):
        raise TritdError(_lib.TRITD_ERR_UNSUPPORTED,
                         "observed (a mask) is implemented for a double D only")
    D = np.asfortranarray(D, dtype=np.float32) if f32 else _fortran(D)
    _size3(D)  # (at most 3-D: refused before the masks are looked at)
    obs, hold = _masks(observed, holdout, D, "D", virtual_shards)
    # E only when asked for (a full tensor more to bring back from the device)
    s = _OneShot(D, r, o.maxIter, opts, A0, B0, C0, tensors=(True, return_E), obs=obs, hold=hold)
    s.solve(_ADMM, "triple_decomp_ADMM", (C.byref(o),), device, (int(patience), int(val_norm)),
            virtual_shards, form="f32" if f32 else None)
    # :68 errHist = errHist(1:k)
    return s.result(s.tensors[:1], s.tensors[1:] * bool(return_E) + [_K] * bool(return_iters))


# the name video_triple_comparison.m:54 calls (unresolvable in the reference)
def triple_decomp_ncvx(X, r, rho, lam, gamma_A, epsilon, p, theta, maxIter, tol, A0=None,
                       B0=None, C0=None, *, device=-1, return_iters=False, observed=None,
                       holdout=None, patience=0, val_norm=2):
    """[A,B,C,O,errHist] of fast_robust_triple_tensor/test.m:1-73 on the GPU
    (the nonconvex variant): outlier ADMM over
    Y = X - O with duals Lambda/Gamma fused into the ALS fit kernel, the
    factors an ALS on X with ridge 1e-12 and the reweighted shrink
    sign(A1).*max(|A1| - gamma_A./(|A1|+epsilon).^(theta-p), 0) on A (:77-92).
    The progress line of :63 goes to the printer every iteration.  On the stop
    test (:65-67) errHist is truncated and O is that of the previous iteration
    (the reference breaks before O = O_new, :71).  fp64, r <= 8.

    ``observed`` (a logical array of X's shape, True = observed) fits the
    observed entries only (tritd_ncvx_masked_f64): X's values at the other
    entries are never used (NaN allowed); there the chain sees the current
    model T, so Y = T, O is exactly 0, the duals stay 0 and errHist counts
    observed entries only, and the factor updates take where(observed, X, T)
    for X.  With every entry observed the result is the unmasked one, bit for
    bit.  For mode-1 shards set the device set (``set_devices``).
    ``observed="nan"``: Omega = ~isnan(X), derived on the device (see
    ``triple_decomp_ADMM``).

    ``holdout`` (a logical array of X's shape; tritd_ncvx_holdout_f64) withholds
    the entries of ``holdout & observed`` from the fit, which is exactly the
    masked one with ``observed & ~holdout``, and scores them in every iteration
    against T of :35: ``valHist(k) = ||H o Omega o (X - T_k)|| / ||H o Omega o X||``
    and ``valHist1(k) = sum|H o Omega o (X - T_k)| / sum|H o Omega o X||``, for
    the factors iteration k started with.  ``val_norm`` (2 or 1) picks the
    history that decides.  The returned tuple then gains a trailing dict with
    ``valHist``, ``valHist1``, ``best_iter`` (the first minimum), ``stop_reason``
    (0 maxIter, 1 the test of :65, 2 patience), ``A_best, B_best, C_best`` (the
    factors iteration best_iter started with; O of the best iterate is not
    kept) and ``holdout_count``.  ``patience = p > 0`` stops the loop at k once
    ``k - best_iter >= p``, like a break of :67."""
    X = _fortran(X)
    _size3(X)
    maxIter = int(maxIter)
    obs, hold = _masks(observed, holdout, X, "X")
    if hold is None and (patience != 0 or val_norm != 2):
        raise ValueError("patience and val_norm need holdout")
    s = _OneShot(X, r, maxIter, None, A0, B0, C0, tensors=(True,), obs=obs, hold=hold)
    s.solve(_NCVX, "triple_decomp_ADMM_outlier",
            (float(rho), float(lam), float(gamma_A), float(epsilon), float(p), float(theta), maxIter,
             float(tol)), device, (int(patience), int(val_norm)))
    return s.result(s.tensors, [_K] * bool(return_iters))


def triple_decomp_ADMM_outlier(*args, **kw):
    """The name the video driver calls (video_triple_comparison.m:54).  In the
    reference it resolves to two different files' internal names: with
    (D, r, opts) it is the ADMM solver (origin_triple_tensor/triple_decomp_ADMM.m:1,
    same maths as the fast one), with the 10 positional arguments of
    fast_robust_triple_tensor/test.m:1 it is the nonconvex variant."""
    if len(args) >= 10:
        return triple_decomp_ncvx(*args, **kw)
    return triple_decomp_ADMM(*args, **kw)


def make_als_opts(opts):
    """opts of triple_decomp_ALS.m:2-3 (only maxIter and tol are read, in
    that order; a missing one raises like MATLAB, everything else is ignored)."""
    o = _lib.Opts()
    for name in ("maxIter", "tol"):
        if _get(opts, name) is None:
            raise KeyError(f"Reference to non-existent field '{name}'.")
    o.maxIter = int(_get(opts, "maxIter"))
    o.tol = float(_get(opts, "tol"))
    o.present = _lib.OPT_MAXITER | _lib.OPT_TOL
    return o


def triple_decomp_ALS(X, r, opts, A0=None, B0=None, C0=None, *, device=-1, return_iters=False,
                      virtual_shards=0, observed=None, holdout=None, patience=0):
    """[A,B,C,errHist] = triple_decomp_ALS(X, r, opts) on the GPU
    (fast_robust_triple_tensor/triple_decomp_ALS.m:1-40).

    ``observed`` (a logical array of X's shape, True = observed) fits the
    observed entries only (tritd_als_masked_f64): X's values at the other
    entries are never used (NaN allowed), the updates see the current model
    there, and errHist counts observed entries only.  For mode-1 shards set
    the device set (``set_devices``), not ``virtual_shards``.
    ``observed="nan"``: Omega = ~isnan(X), derived on the device (see
    ``triple_decomp_ADMM``).

    ``holdout`` (a logical array of X's shape; tritd_als_holdout_f64) withholds
    the entries of ``holdout & observed`` from the fit, which is exactly the
    masked one with ``observed & ~holdout``, and scores them every iteration in
    the fit kernel's own pass: ``valHist(k) = ||H o Omega o (X - Xhat)|| /
    ||H o Omega o X||`` for the factors iteration k started with.  The returned
    tuple then gains a trailing dict with ``valHist``, ``best_iter`` (the first
    minimum of valHist), ``stop_reason`` (0 maxIter, 1 the test of :20,
    2 patience), ``A_best, B_best, C_best`` (the factors iteration best_iter
    started with) and ``holdout_count``.  ``patience = p > 0`` stops the loop
    at k once ``k - best_iter >= p``.

    The initial factors are drawn here in the order of :8-10 unless given
    (MATLAB's randn is not reproducible outside MATLAB).  The progress line of
    :17-19 goes to the printer (``tritd.set_printer``; stdout by default).
    ``return_iters`` adds k; ``virtual_shards=P`` runs the mode-1 sharded
    schedule as P shards on one device.  fp64, r <= 8."""
    o = make_als_opts(opts)
    X = _fortran(X)
    _size3(X)
    obs, hold = _masks(observed, holdout, X, "X", virtual_shards)
    s = _OneShot(X, r, o.maxIter, opts, A0, B0, C0, tensors=(), obs=obs, hold=hold, l1=False)
    s.solve(_ALS, "triple_decomp_ALS", (C.byref(o),), device, (int(patience),), virtual_shards)
    return s.result((), [_K] * bool(return_iters))  # :21 errHist = errHist(1:k)


def triple_product(A, B, C_, model="cp"):
    """Xhat = triple_product(A, B, C)  (triple_product.m:1-7).  model='qi': Qi's
    3-index product sum_{p,q,s} A(i,q,s)B(p,j,s)C(p,q,t)
    (origin_triple_tensor/triple_product.m:8-19, buildF.m:2-6)."""
    A = _fortran(A)
    B = _fortran(B)
    C_ = _fortran(C_)
    n1, r, _ = _size3(A)
    n2 = _size3(B)[1]
    n3 = _size3(C_)[2]
    X = np.zeros((n1, n2, n3), order="F")
    fn = lib.tritd_triple_product_qi_f64 if model_code(model) else lib.tritd_triple_product_f64
    check(fn(_ptr(A), _ptr(B), _ptr(C_), n1, n2, n3, r, _ptr(X)))
    return X


def unfold(X, mode):
    """Xn = unfold(X, mode)  (unfold.m:1-13)."""
    X = _fortran(X)
    n1, n2, n3 = _size3(X)
    shapes = {1: (n1, n2 * n3), 2: (n2, n1 * n3), 3: (n3, n1 * n2)}
    out = np.zeros(shapes.get(int(mode), (1,)), order="F")
    check(lib.tritd_unfold_f64(_ptr(X), n1, n2, n3, int(mode), _ptr(out)))
    return out


def soft_threshold(X, lam):
    """O = soft_threshold(X, lam)  (soft_threshold.m:1-2)."""
    X = _fortran(X)
    Y = np.zeros_like(X, order="F")
    check(lib.tritd_soft_threshold_f64(_ptr(X), X.size, float(lam), _ptr(Y)))
    return Y


def evaluate(X, gt, mask=None):
    """[rmse, nrmse] = evaluate(X, gt, mask)  (traffic_triple_comparison.m:194-202):
    rmse = norm(X(mask) - gt(:)), nrmse = rmse / norm(gt(:)); mask None means
    true(size(X)).  gt holds the masked entries in column-major order."""
    X = _fortran(X)
    gt = _fortran(gt)
    m = None
    if mask is not None:
        mk = np.asarray(mask)
        if mk.shape != X.shape:
            raise ValueError("Index exceeds the number of array elements (mask shape differs).")
        m = np.asfortranarray(mk != 0).view(np.uint8)
    rmse, nrmse = C.c_double(0), C.c_double(0)
    check(lib.tritd_evaluate_f64(_ptr(X), X.size, _ptr(gt), gt.size, _ptr(m) if m is not None else None,
                                 C.byref(rmse), C.byref(nrmse)))
    return rmse.value, nrmse.value


def quality_ybz(imagery1, imagery2, per_frame=False):
    """[psnr, ssim] = quality_ybz(imagery1, imagery2): mean over the frames
    (dims 3.. folded) of psnr_index and ssim_index (dynamic range [0, 255])."""
    X1 = _fortran(imagery1)
    X2 = _fortran(imagery2)
    if X1.shape != X2.shape:
        raise ValueError("imagery1 and imagery2 must have the same size")
    n1 = X1.shape[0]
    n2 = X1.shape[1] if X1.ndim > 1 else 1
    nf = max(X1.size // max(n1 * n2, 1), 1)
    p, s = C.c_double(0), C.c_double(0)
    pf = np.zeros(nf)
    sf = np.zeros(nf)
    check(lib.tritd_quality_f64(_ptr(X1), _ptr(X2), n1, n2, nf, C.byref(p), C.byref(s), _ptr(pf),
                                _ptr(sf)))
    if per_frame:
        return p.value, s.value, pf, sf
    return p.value, s.value


def _label_bytes(groundtruth, shape, what="groundtruth"):
    """CDnet labels as bytes.  Only 255 (motion) and 170 (unknown) are ever
    compared (video_triple_comparison.m:342-343), so an array of another type
    keeps exactly those two values and becomes 0 elsewhere.  A uint8 array
    whose strides are those of a column-major array with a larger leading
    dimension (rows i0:i1 of the whole ground truth) is used where it lies.
    -> (array to keep alive, leading dimension)"""
    G = np.asarray(groundtruth)
    if tuple(G.shape) != tuple(shape):
        raise ValueError(f"{what} must have the shape {tuple(shape)}, got {tuple(G.shape)}")
    if G.dtype != np.uint8:
        G = np.where(G == 255, 255, np.where(G == 170, 170, 0)).astype(np.uint8)
    if G.ndim == 3 and G.size and G.strides[0] == 1:
        ld = G.strides[1]
        if ld >= G.shape[0] and G.strides == (1, ld, ld * G.shape[1]):
            return G, int(ld)
    G = np.asfortranarray(G)
    return G, int(G.shape[0]) if G.ndim else 1


def foreground_scores(counts, numel):
    """The scores of eval (video_triple_comparison.m:356-365) from per-frame
    counts (nf, 4) in the order TP, FP, FN, TN: dict(total=int64[4], precision,
    recall, f1, pwc), in double; 0/0 is NaN as in MATLAB.  Host arithmetic in
    the library (tritd_foreground_scores): no device is needed."""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.int64).reshape(-1, 4))
    total = np.zeros(4, dtype=np.int64)
    v = [C.c_double(0) for _ in range(4)]
    check(lib.tritd_foreground_scores(_ptr(c), c.shape[0], int(numel), _ptr(total),
                                      *(C.byref(x) for x in v)))
    return dict(total=total, precision=v[0].value, recall=v[1].value, f1=v[2].value,
                pwc=v[3].value)


def foreground_eval(F, groundtruth=None, thr=50.0):
    """eval(origin, groundtruth, background, foreground) of
    video_triple_comparison.m:316-371 on the GPU: ``mask = abs(F) > thr``
    (strict; NaN False) and, with a ground truth of CDnet labels (255 = motion,
    170 = unknown), the per-frame ``counts`` (nf, 4) = TP, FP, FN, TN with
    their ``total`` and ``precision``, ``recall``, ``f1``, ``pwc``.  F is
    float64 or float32 (anything else is taken as float64); dimensions past
    the second are folded into frames, as ``quality_ybz`` does.  Without a
    ground truth only ``mask`` is returned."""
    F = np.asarray(F)
    f32 = F.dtype == np.float32
    F = np.asfortranarray(F, dtype=np.float32 if f32 else np.float64)
    if F.ndim == 0:
        F = F.reshape(1)
    n1 = F.shape[0]
    n2 = F.shape[1] if F.ndim > 1 else 1
    nf = max(F.size // max(n1 * n2, 1), 1)
    G = None
    if groundtruth is not None:
        G = np.asfortranarray(_label_bytes(groundtruth, F.shape)[0])
    mask = np.zeros(F.shape, dtype=np.uint8, order="F")
    counts = np.zeros((nf, 4), dtype=np.int64)
    fn = lib.tritd_foreground_f32 if f32 else lib.tritd_foreground_f64
    check(fn(_ptr(F), _ptr(G), n1, n2, nf, float(thr), _ptr(mask), _ptr(counts)))
    out = dict(mask=mask.view(np.bool_))
    if G is not None:
        out.update(counts=counts, **foreground_scores(counts, F.size))
    return out


def _in_place(a, shape, dtype):
    """``a`` as a column-major (nl, n2, n3) array of ``dtype`` with a leading
    dimension: rows i0:i1 of a whole column-major tensor are used where they
    lie (their strides give ld), anything else is copied.
    -> (array to keep alive, leading dimension in elements)"""
    a = np.asarray(a)
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected the shape {tuple(shape)}, got {tuple(a.shape)}")
    es = np.dtype(dtype).itemsize
    if a.dtype == np.dtype(dtype) and a.ndim == 3 and a.size and a.strides[0] == es:
        ld = a.strides[1] // es
        if ld >= a.shape[0] and a.strides == (es, ld * es, ld * es * a.shape[1]):
            return a, int(ld)
    a = np.asfortranarray(a, dtype=dtype)
    return a, int(a.shape[0])


def report_scores(sums, frame_sq, frame_ssim, n1, n2):
    """The eight figures of video_triple_comparison.m:64-67 from the raw parts
    of ``Session.report`` (tritd_session_report), on the host: a caller with
    several shards adds their ``sums`` and ``frame_sq`` first.  evaluate
    (:290-298): rmse = sqrt(S0), nrmse = sqrt(S0)/sqrt(S1), srmse/snrmse from
    S2, S3, trmse/tnrmse from S4, S5; 0/0 is NaN, as MATLAB gives for an empty
    gt.  psnr_index: psnr_frames = 10 log10(255^2 / (frame_sq / (n1 n2))), psnr
    and ssim the means over the frames (quality_ybz).  ``frame_ssim`` None:
    ssim is NaN and ssim_frames None.  ``n1, n2``: the size of a whole frame."""
    S = np.asarray(sums, dtype=np.float64).reshape(6)
    fsq = np.asarray(frame_sq, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        root = np.sqrt(S)
        out = dict(rmse=float(root[0]), nrmse=float(root[0] / root[1]),
                   srmse=float(root[2]), snrmse=float(root[2] / root[3]),
                   trmse=float(root[4]), tnrmse=float(root[4] / root[5]))
        pf = 10.0 * np.log10(255.0 ** 2 / (fsq / float(n1 * n2)))
    out.update(psnr=float(np.mean(pf)), psnr_frames=pf)
    if frame_ssim is None:
        out.update(ssim=float("nan"), ssim_frames=None)
    else:
        sf = np.asarray(frame_ssim, dtype=np.float64).reshape(-1)
        out.update(ssim=float(np.mean(sf)), ssim_frames=sf)
    return out


def _design(which, P, Q, nP, nQ, r):
    out = np.zeros((r * r, nP * nQ), order="F")
    check(lib.tritd_build_design_f64(which.encode(), _ptr(P), _ptr(Q), nP, nQ, r, _ptr(out)))
    return out


def buildF(B, C_):
    """F = buildF(B, C)  (buildF.m:1-22)."""
    B = _fortran(B)
    C_ = _fortran(C_)
    r, n2, _ = _size3(B)
    return _design("F", B, C_, n2, _size3(C_)[2], r)


def buildG(A, C_):
    """G = buildG(A, C)  (buildG.m:1-22)."""
    A = _fortran(A)
    C_ = _fortran(C_)
    n1, r, _ = _size3(A)
    return _design("G", A, C_, n1, _size3(C_)[2], r)


def buildH(A, B):
    """H = buildH(A, B)  (buildH.m:1-22)."""
    A = _fortran(A)
    B = _fortran(B)
    n1, r, _ = _size3(A)
    return _design("H", A, B, n1, _size3(B)[1], r)


# ---------------------------------------------------------------------------
# Sessions: device-resident loop (bench, multi-GPU)
# ---------------------------------------------------------------------------
def _marshal_shard(data, device_ptr, ld, rows, observed, holdout, what, dtype, flags):
    """A shard's data and masks for a session creator: a host array (made
    column-major ``dtype``; the masks logical arrays of its shape) or a device
    pointer (the masks device pointers too), ``observed`` possibly "nan".
    -> (data pointer, ld, observed pointer, holdout pointer, flags, the host
    arrays to keep alive over the call)."""
    if device_ptr is not None:
        ld = ld if ld is not None else rows
        hptr = C.c_void_p(int(holdout)) if holdout is not None else None
        return (C.c_void_p(int(device_ptr)), int(ld), _device_mask(observed), hptr,
                flags | _lib.SESSION_D_ON_DEVICE, ())
    data = np.asfortranarray(data, dtype=dtype)
    ld = ld if ld is not None else data.shape[0]
    obs = _observed_bytes(observed, data.shape, what) if observed is not None else None
    hold = _observed_bytes(holdout, data.shape, what, "holdout") if holdout is not None else None
    return _ptr(data), int(ld), _ptr(obs), _ptr(hold), flags, (data, obs, hold)


class _SessionBase:
    """What ``Session`` and ``AlsSession`` share: the creation of a shard's
    session and the calls that differ only in the C symbol's prefix."""

    _prefix = ""  # "tritd_session_" / "tritd_als_session_"

    def _fn(self, name):
        return getattr(lib, self._prefix + name)

    def _create(self, r, o, start, n1, n2, n3, i0, i1, data, device_ptr, ld, device, comm, observed,
                holdout, what, dtype=np.float64, flags=0, holdout_args=(), tail=(), form=None):
        """Create the session of form "" (plain), "masked" or "holdout" (what
        the masks imply) unless ``form`` names another creator.  ``o``: the
        tritd_opts; ``holdout_args`` follow it in a holdout creator; ``tail``
        follows the flags."""
        i1 = n1 if i1 is None else i1
        start = [_fortran(a) for a in start]
        dptr, ld, optr, hptr, flags, keep = _marshal_shard(data, device_ptr, ld, i1 - i0, observed,
                                                           holdout, what, dtype, flags)
        self.n1, self.n2, self.n3, self.i0, self.i1, self.r = n1, n2, n3, i0, i1, r
        self.maxIter = o.maxIter
        if form is None:
            form = "holdout" if hptr is not None else "masked" if optr is not None else ""
        args = [C.byref(self._s), int(device), dptr]
        if form:
            args.append(optr)
        if hptr is not None:
            args.append(hptr)
        args += [ld, n1, n2, n3, i0, i1, r, C.byref(o)]
        if hptr is not None:
            args += holdout_args
        args += [_ptr(a) for a in start]
        args += [comm.handle if comm is not None else None, flags, *tail]
        # (`keep` holds the host arrays until the creator has copied the shard)
        check(self._fn("create_" + form if form else "create")(*args))

    def _factors(self):
        """zeroed A, B, C of the whole problem's shapes (column-major)"""
        r, n1, n2, n3 = self.r, self.n1, self.n2, self.n3
        return (np.zeros((n1, r, r), order="F"), np.zeros((r, n2, r), order="F"),
                np.zeros((r, r, n3), order="F"))

    def mask_info(self):
        """(whether the session has a mask, observed entries of its shard)"""
        m, c = _lib.i32(0), _lib.i64(0)
        check(self._fn("mask_info")(self._s, C.byref(m), C.byref(c)))
        return bool(m.value), c.value

    def get_best(self):
        """The factors of the best iterate (after iteration best_iter for the
        ADMM, the ones iteration best_iter started with for the ALS and the
        nonconvex solver), shaped like those of ``get()``: tritd_session_get_best
        / tritd_als_session_get_best."""
        A, B, Cf = self._factors()
        check(self._fn("get_best")(self._s, _ptr(A), _ptr(B), _ptr(Cf)))
        return dict(A=A, B=B, C=Cf)

    def foreground(self, thr=50.0, groundtruth=None, *, return_mask=True, gt_device_ptr=None,
                   mask_device_ptr=None, ldG=None, ldP=None):
        """eval of video_triple_comparison.m:316-371 on the session's own O
        (tritd_session_foreground / tritd_als_session_foreground): the O that
        ``get()`` / ``get_O()`` would return now, thresholded on the device
        where the session keeps it, so O is never rebuilt, converted or
        downloaded.  -> dict(mask=bool (nl, n2, n3) column-major, counts=int64
        (n3, 4) as TP, FP, FN, TN of the shard's rows, total, precision, recall,
        f1, pwc); the mask is absent with ``return_mask=False``, the counts and
        scores without a ground truth.  ``groundtruth``: the labels of the
        shard's rows (nl, n2, n3), e.g. ``G[i0:i1]`` of the whole ground truth.
        ``gt_device_ptr`` / ``mask_device_ptr`` (with ``ldG`` / ``ldP``, default
        nl) take the labels from and write the mask to device memory instead
        (TRITD_FG_DEVICE); the mask is then not returned.  The session's state
        is untouched: a ``run`` after it continues as without it."""
        nl, n2, n3 = self.i1 - self.i0, self.n2, self.n3
        counts = np.zeros((n3, 4), dtype=np.int64)
        mask = G = None
        if gt_device_ptr is not None or mask_device_ptr is not None:
            if groundtruth is not None:
                raise ValueError("groundtruth (host) with device pointers: pass gt_device_ptr")
            _lib.check_one_runtime("foreground(gt_device_ptr=...)")
            gptr = C.c_void_p(int(gt_device_ptr)) if gt_device_ptr is not None else None
            pptr = C.c_void_p(int(mask_device_ptr)) if mask_device_ptr is not None else None
            ldG = nl if ldG is None else int(ldG)
            ldP = nl if ldP is None else int(ldP)
            flags, counted = _lib.FG_DEVICE, gptr is not None
        else:
            gptr, ldG = None, nl
            if groundtruth is not None:
                G, ldG = _label_bytes(groundtruth, (nl, n2, n3))
                gptr = _ptr(G)
            if return_mask:
                mask = np.zeros((nl, n2, n3), dtype=np.uint8, order="F")
            pptr, ldP, flags, counted = _ptr(mask), nl, 0, G is not None
        check(self._fn("foreground")(self._s, float(thr), gptr, ldG, pptr, ldP, _ptr(counts), flags))
        out = {}
        if mask is not None:
            out["mask"] = mask.view(np.bool_)
        if counted:
            out.update(counts=counts, **foreground_scores(counts, nl * n2 * n3))
        return out

    def report(self, X=None, missing=None, *, ssim=True, x_device_ptr=None,
               missing_device_ptr=None, ldX=None, ldM=None):
        """The figures video_triple_comparison.m:64-67 prints, from the
        session's resident tensors (tritd_session_report /
        tritd_als_session_report): with L the triple product of
        the current factors and O what ``get()`` / ``get_O()`` would return now
        (0 for a plain ALS session and before the first ADMM iteration),
        ``rmse, nrmse`` of L on the missing entries, ``srmse, snrmse`` of O on
        the others, ``trmse, tnrmse`` of L + O on all, ``psnr, ssim`` of L
        against X with ``psnr_frames, ssim_frames``, and the raw ``sums`` (6)
        and ``frame_sq`` (n3) they come from (``report_scores``; a caller with
        several shards adds those).  Neither L nor O is materialised or
        downloaded.  ``X``: the original tensor of the shard's rows (nl, n2,
        n3), e.g. ``X[i0:i1]`` of the whole tensor, used where it lies;
        ``missing``: a logical array of the same shape, True = missing (None:
        nothing is).  ``x_device_ptr`` / ``missing_device_ptr`` (with ``ldX`` /
        ``ldM``, default nl) take them from device memory instead
        (TRITD_REPORT_DEVICE).  ``ssim=False`` skips SSIM and its scratch; a
        session that does not hold all rows must (TRITD_ERR_ARG otherwise).
        fp64 sessions.  The session's state is untouched."""
        nl, n2, n3 = self.i1 - self.i0, self.n2, self.n3
        if x_device_ptr is not None:
            if X is not None or missing is not None:
                raise ValueError("X / missing (host) with x_device_ptr: pass device pointers")
            _lib.check_one_runtime("report(x_device_ptr=...)")
            xptr = C.c_void_p(int(x_device_ptr))
            mptr = C.c_void_p(int(missing_device_ptr)) if missing_device_ptr is not None else None
            ldX = nl if ldX is None else int(ldX)
            ldM = nl if ldM is None else int(ldM)
            flags, keep = _lib.REPORT_DEVICE, ()
        else:
            if X is None or missing_device_ptr is not None:
                raise ValueError("report needs X, or x_device_ptr with missing_device_ptr")
            Xa, ldX = _in_place(X, (nl, n2, n3), np.float64)
            xptr, mptr, ldM, keep = _ptr(Xa), None, nl, (Xa,)
            if missing is not None:
                m = np.asarray(missing)
                if m.dtype.itemsize != 1:
                    m = m != 0
                Ma, ldM = _in_place(m.view(np.uint8), (nl, n2, n3), np.uint8)
                mptr, keep = _ptr(Ma), (Xa, Ma)
            flags = 0
        sums, fsq = np.zeros(6), np.zeros(n3)
        fss = np.zeros(n3) if ssim else None
        check(self._fn("report")(self._s, xptr, ldX, mptr, ldM, _ptr(sums), _ptr(fsq), _ptr(fss),
                                 flags))
        del keep
        out = report_scores(sums, fsq, fss, self.n1, n2)
        out.update(sums=sums, frame_sq=fsq)
        return out

    def run(self, iters):
        check(self._fn("run")(self._s, int(iters)))

    def sync(self):
        d, s = _lib.i32(0), _lib.i32(0)
        check(self._fn("sync")(self._s, C.byref(d), C.byref(s)))
        return d.value, bool(s.value)

    def flags(self):
        """TRITD_FLAG_* raised so far (read at each sync)."""
        f = C.c_uint32(0)
        check(self._fn("flags")(self._s, C.byref(f)))
        return f.value

    def close(self):
        if self._s:
            self._fn("destroy")(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Session(_SessionBase):
    """One mode-1 shard [i0, i1) of an n1 x n2 x n3 problem on one GPU.

    D is either a host numpy array holding the shard (column-major, leading
    dimension ldD) or, with ``d_device_ptr``, a device pointer.  ``dtype``
    float32 (or a float32 D) selects the single-class path.  ``probe``
    (default True) times candidate placements of the tensor pool at creation
    and keeps the fastest (TRITD_SESSION_PROBE): worth it for a session that
    runs hundreds of iterations, not for one solve.

    ``observed`` is the mask of the shard (tritd_session_create_masked): with
    a host D a logical array of D's shape, with ``d_device_ptr`` a device
    pointer to bytes laid out like D (fibres ldD bytes apart); in either case
    ``"nan"`` for Omega = ~isnan(D), derived on the device.  float64 only.

    ``holdout`` (given like ``observed``), ``patience`` and ``val_norm`` make it
    a holdout session (tritd_session_create_holdout; see
    ``triple_decomp_ADMM``): ``get()`` then also returns ``valHist``,
    ``valHist1``, ``best_iter`` and ``stop_reason`` (so does ``get_val()``,
    without the tensors), ``get_best()`` the factors after iteration best_iter,
    and ``holdout_info()`` the held-out count of the shard, ``||H o Omega o D||``
    and ``sum |H o Omega o D|``."""

    _prefix = "tritd_session_"

    def __init__(self, r, opts, A0, B0, C0, *, n1, n2, n3, i0=0, i1=None, D=None,
                 d_device_ptr=None, ldD=None, device=0, comm=None, dtype=None, probe=True,
                 observed=None, holdout=None, patience=0, val_norm=2):
        self._s = C.c_void_p()
        self._holdout = holdout is not None
        o = make_opts(opts)
        if dtype is None:
            dtype = np.asarray(D).dtype if D is not None else np.float64
        self.f32 = np.dtype(dtype) == np.float32
        flags = _lib.SESSION_F32 if self.f32 else 0
        if probe:
            flags |= _lib.SESSION_PROBE
        if d_device_ptr is not None:
            _lib.check_one_runtime("Session(d_device_ptr=...)")
        self._create(r, o, (A0, B0, C0), n1, n2, n3, i0, i1, D, d_device_ptr, ldD, device, comm,
                     observed, holdout, "D", np.float32 if self.f32 else np.float64, flags,
                     (int(patience), int(val_norm)))


    def holdout_info(self):
        """(held-out entries of the shard, ||H o Omega o D|| and sum |H o Omega o D|
        over all shards)"""
        c, nrm, s1 = _lib.i64(0), C.c_double(0), C.c_double(0)
        check(lib.tritd_session_holdout_info(self._s, C.byref(c), C.byref(nrm), C.byref(s1)))
        return c.value, nrm.value, s1.value

    def get_val(self):
        """valHist, valHist1, best_iter, stop_reason: tritd_session_get_val."""
        vh, vh1 = np.zeros(max(self.maxIter, 1)), np.zeros(max(self.maxIter, 1))
        best, why = _lib.i32(0), _lib.i32(0)
        check(lib.tritd_session_get_val(self._s, _ptr(vh), _ptr(vh1), C.byref(best), C.byref(why)))
        k = self.sync()[0]
        return dict(valHist=vh[:k].copy(), valHist1=vh1[:k].copy(), best_iter=best.value,
                    stop_reason=why.value)


    def holdout_ms(self):
        """(score kernel ms, ms from the end of K5 to the end of the iteration)
        per timed iteration: tritd_session_holdout_ms."""
        a, b = C.c_double(0), C.c_double(0)
        check(lib.tritd_session_holdout_ms(self._s, C.byref(a), C.byref(b)))
        return a.value, b.value


    def get(self):
        n2, n3 = self.n2, self.n3
        nl = self.i1 - self.i0
        A, B, Cf = self._factors()
        dt = np.float32 if self.f32 else np.float64
        O = np.zeros((nl, n2, n3), order="F", dtype=dt)
        E = np.zeros((nl, n2, n3), order="F", dtype=dt)
        eh = np.zeros(max(self.maxIter, 1))
        k = _lib.i32(0)
        fn = lib.tritd_session_get_f32 if self.f32 else lib.tritd_session_get
        check(fn(self._s, _ptr(A), _ptr(B), _ptr(Cf), _ptr(O), _ptr(E), nl, _ptr(eh), C.byref(k)))
        _lib.warn_flags(self.flags(), "Session")
        out = dict(A=A, B=B, C=Cf, O=O, E=E, errHist=eh[: k.value].copy(), k=k.value)
        if self._holdout:
            out.update(self.get_val())
        return out

    def foreground_ms(self):
        """ms of the kernel of the last ``foreground`` made with ``set_timing``
        on (HIP events around its launch): tritd_session_foreground_ms."""
        ms = C.c_double(0)
        check(lib.tritd_session_foreground_ms(self._s, C.byref(ms)))
        return ms.value

    def report_ms(self):
        """ms of the kernels of the last ``report`` made with ``set_timing``
        on (HIP events around them): tritd_session_report_ms."""
        ms = C.c_double(0)
        check(lib.tritd_session_report_ms(self._s, C.byref(ms)))
        return ms.value

    def rre_parts(self, dX_ptr, ldX):
        _lib.check_one_runtime("Session.rre_parts")
        num, den = C.c_double(0), C.c_double(0)
        fn = lib.tritd_session_rre_parts_f32 if self.f32 else lib.tritd_session_rre_parts
        check(fn(self._s, C.c_void_p(int(dX_ptr)), int(ldX), C.byref(num), C.byref(den)))
        return num.value, den.value

    def comm_ms(self):
        """(mean all-reduce ms per timed iteration, all-reduces per iteration)
        — set_timing(True) with a communicator (tritd_session_comm_ms)."""
        ms, n = C.c_double(0), _lib.i32(0)
        check(lib.tritd_session_comm_ms(self._s, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def probe(self):
        """(probe ms of each candidate tensor pool, index kept)"""
        cap = 64  # up to three rounds of candidates (solver.cpp probe_pool)
        ms = (C.c_double * cap)()
        n, k = _lib.i32(0), _lib.i32(0)
        check(lib.tritd_session_probe(self._s, ms, cap, C.byref(n), C.byref(k)))
        return [ms[i] for i in range(min(n.value, cap))], k.value

    def counters(self):
        """(E tiles stored densely over all fused-update launches, tiles per launch)"""
        a, b = _lib.i64(0), _lib.i64(0)
        check(lib.tritd_session_counters(self._s, C.byref(a), C.byref(b)))
        return a.value, b.value

    def k5_profile(self):
        """(dense N-streams per fused-update launch, compact-E slot accesses per tile)"""
        a, b = _lib.i32(0), _lib.i32(0)
        check(lib.tritd_session_k5_profile(self._s, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_timing(self, on=True):
        """on: False/0 off, True/1 events around the iteration, K2 and K5,
        "k5"/2 around K5 only (fewer stream markers inside a timed region)."""
        level = 2 if on == "k5" else int(on)
        check(lib.tritd_session_set_timing(self._s, level))

    def kernel_ms(self):
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        n = _lib.i32(0)
        check(lib.tritd_session_kernel_ms(self._s, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return dict(fused_update=a.value, mode3=b.value, iteration=c.value, samples=n.value)



class AlsSession(_SessionBase):
    """Steppable device-resident triple_decomp_ALS on one mode-1 shard
    (bench; one process per GPU with ``comm``).  ``quiet`` drops the
    every-5-iterations progress line and its host synchronisation.

    ``observed`` is the mask of the shard (tritd_als_session_create_masked):
    with a host X a logical array of X's shape, with ``x_device_ptr`` a device
    pointer to bytes laid out like X (fibres ldX bytes apart); in either case
    ``"nan"`` for Omega = ~isnan(X), derived on the device.

    ``ncvx=dict(rho=, lam=, gamma_A=, epsilon=, p=, theta=)`` turns the session,
    masked or not, into the nonconvex solver of test.m:1-73
    (tritd_als_session_set_ncvx; ``triple_decomp_ncvx`` stepped): ``get_O``
    then returns the shard's O, and with ``quiet=False`` the progress line
    comes every iteration.

    ``holdout`` (given like ``observed``) and ``patience`` make it a holdout
    session (tritd_als_session_create_holdout; see ``triple_decomp_ALS``):
    ``get()`` then also returns ``valHist``, ``best_iter`` and ``stop_reason``,
    ``get_best()`` the factors iteration best_iter started with, and
    ``holdout_info()`` the held-out count of the shard and ``||H o Omega o X||``.
    ``ncvx`` with ``holdout`` is refused (TRITD_ERR_UNSUPPORTED)."""

    _prefix = "tritd_als_session_"

    def __init__(self, r, opts, A0, B0, C0, *, n1, n2, n3, i0=0, i1=None, X=None,
                 x_device_ptr=None, ldX=None, device=0, comm=None, quiet=True, observed=None,
                 ncvx=None, holdout=None, patience=0):
        self._s = C.c_void_p()
        self._holdout = holdout is not None
        if ncvx is not None:
            ncvx = [float(ncvx[k]) for k in ("rho", "lam", "gamma_A", "epsilon", "p", "theta")]
        self._create(r, make_als_opts(opts), (A0, B0, C0), n1, n2, n3, i0, i1, X, x_device_ptr, ldX,
                     device, comm, observed, holdout, "X", holdout_args=(int(patience),),
                     tail=(int(bool(quiet)),))
        if ncvx is not None:
            self.set_ncvx(*ncvx)

    def set_ncvx(self, rho, lam, gamma_A, epsilon, p, theta):
        """tritd_als_session_set_ncvx: before the first ``run``."""
        check(lib.tritd_als_session_set_ncvx(self._s, float(rho), float(lam), float(gamma_A),
                                             float(epsilon), float(p), float(theta)))

    def get_O(self):
        """O of the shard (rows i0..i1-1), tritd_als_session_get_O: that of
        iteration k-1 when the stop test broke the loop at k, else the last;
        exactly 0 where unobserved."""
        O = np.zeros((self.i1 - self.i0, self.n2, self.n3), order="F")
        check(lib.tritd_als_session_get_O(self._s, _ptr(O), self.i1 - self.i0))
        return O


    def holdout_info(self):
        """(held-out entries of the shard, ||H o Omega o X|| over all shards)"""
        c, nrm = _lib.i64(0), C.c_double(0)
        check(lib.tritd_als_session_holdout_info(self._s, C.byref(c), C.byref(nrm)))
        return c.value, nrm.value



    def get(self):
        A, B, Cf = self._factors()
        eh = np.zeros(max(self.maxIter, 1))
        k = _lib.i32(0)
        check(lib.tritd_als_session_get(self._s, _ptr(A), _ptr(B), _ptr(Cf), _ptr(eh), C.byref(k)))
        _lib.warn_flags(self.flags(), "AlsSession")
        out = dict(A=A, B=B, C=Cf, errHist=eh[: k.value].copy(), k=k.value)
        if self._holdout:
            vh = np.zeros(max(self.maxIter, 1))
            best, why = _lib.i32(0), _lib.i32(0)
            check(lib.tritd_als_session_get_val(self._s, _ptr(vh), C.byref(best), C.byref(why)))
            out.update(valHist=vh[: k.value].copy(), best_iter=best.value, stop_reason=why.value)
        return out

    def set_timing(self, on=True):
        check(lib.tritd_als_session_set_timing(self._s, int(bool(on))))

    def kernel_ms(self):
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        n = _lib.i32(0)
        check(lib.tritd_als_session_kernel_ms(self._s, C.byref(a), C.byref(b), C.byref(c),
                                              C.byref(n)))
        return dict(fit=a.value, mode3=b.value, iteration=c.value, samples=n.value)



class NcvxSession(AlsSession):
    """Steppable nonconvex solver of test.m:1-73 with a holdout
    (tritd_als_session_create_ncvx_holdout; ``triple_decomp_ncvx(holdout=)``
    stepped) on one mode-1 shard.  ``ncvx=dict(rho=, lam=, gamma_A=, epsilon=,
    p=, theta=)``; ``opts`` carries maxIter and tol; X, ``observed`` and
    ``holdout`` are given as for ``AlsSession`` (host arrays, or device pointers
    with ``x_device_ptr`` and ``ldX``).  ``get()`` also returns ``valHist``,
    ``valHist1``, ``best_iter`` and ``stop_reason`` (``get_val()`` returns those
    alone), ``get_best()`` the factors iteration best_iter started with,
    ``get_O()`` the shard's O, ``holdout_info()`` the held-out count of the
    shard and ``||H o Omega o X||``, ``holdout_ms()`` the score kernel's time."""

    def __init__(self, r, opts, A0, B0, C0, *, ncvx, holdout, n1, n2, n3, i0=0, i1=None, X=None,
                 x_device_ptr=None, ldX=None, device=0, comm=None, quiet=True, observed=None,
                 patience=0, val_norm=2):
        self._s = C.c_void_p()
        self._holdout = True
        if holdout is None:
            raise ValueError("NcvxSession needs holdout (AlsSession(ncvx=) runs without one)")
        prm = [float(ncvx[k]) for k in ("rho", "lam", "gamma_A", "epsilon", "p", "theta")]
        self._create(r, make_als_opts(opts), (A0, B0, C0), n1, n2, n3, i0, i1, X, x_device_ptr, ldX,
                     device, comm, observed, holdout, "X",
                     holdout_args=(int(patience), int(val_norm), *prm), tail=(int(bool(quiet)),),
                     form="ncvx_holdout")

    def get_val(self):
        """dict(valHist, valHist1, best_iter, stop_reason): tritd_als_session_get_val2."""
        d, _ = self.sync()
        vh, vh1 = np.zeros(max(self.maxIter, 1)), np.zeros(max(self.maxIter, 1))
        best, why = _lib.i32(0), _lib.i32(0)
        check(lib.tritd_als_session_get_val2(self._s, _ptr(vh), _ptr(vh1), C.byref(best),
                                             C.byref(why)))
        return dict(valHist=vh[:d].copy(), valHist1=vh1[:d].copy(), best_iter=best.value,
                    stop_reason=why.value)

    def get(self):
        out = super().get()
        out["valHist1"] = self.get_val()["valHist1"]
        return out

    def holdout_ms(self):
        """dict(score=, tail=): ms per timed iteration in the score kernel, and
        from the end of the fit kernel to the start of the A update:
        tritd_als_session_holdout_ms."""
        a, b = C.c_double(0), C.c_double(0)
        check(lib.tritd_als_session_holdout_ms(self._s, C.byref(a), C.byref(b)))
        return dict(score=a.value, tail=b.value)


class Comm:
    """RCCL communicator owned by libtritd (one process per GPU), or — with
    :meth:`host` — a host transport that hands every all-reduce to a Python
    function (tritd_comm_create_host)."""

    def __init__(self, unique_id: bytes, nranks, rank, device):
        self.handle = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(lib.tritd_comm_create(C.byref(self.handle), buf, int(nranks), int(rank), int(device)))

    @classmethod
    def host(cls, fn, nranks, rank, device):
        """fn(buf, op) all-reduces the float64 numpy array `buf` in place over
        the ranks (op 0: sum, 1: max).  Every all-reduce of a session drains
        its stream first: a correctness transport (several ranks on one GPU,
        hosts with their own collectives), not the fast path."""
        self = cls.__new__(cls)
        self.handle = C.c_void_p()

        def cb(buf, count, op, user):
            try:
                if count > 0:
                    fn(np.ctypeslib.as_array(buf, shape=(int(count),)), int(op))
                return 0
            except Exception:  # reported to the library as a failed collective
                import traceback
                traceback.print_exc()
                return 1

        self._cb = _lib.ALLREDUCE_FN(cb)  # kept alive with the comm
        check(lib.tritd_comm_create_host(C.byref(self.handle), self._cb, None, int(nranks),
                                         int(rank), int(device)))
        return self

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(lib.tritd_comm_unique_id(buf))
        return buf.raw

    def info(self):
        """(nranks, rank, transport) as the communicator reports them
        (RCCL: ncclCommCount / ncclCommUserRank); transport 'rccl' or 'host'."""
        n, me, tr = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib.tritd_comm_info(self.handle, C.byref(n), C.byref(me), C.byref(tr)))
        return n.value, me.value, ("rccl" if tr.value == 0 else "host")

    def close(self):
        if self.handle:
            lib.tritd_comm_destroy(self.handle)
            self.handle = C.c_void_p()


__all__ = ["triple_decomp_ADMM", "triple_decomp_ADMM_outlier", "triple_decomp_ALS", "AlsSession",
           "NcvxSession",
           "triple_decomp_ncvx",
           "make_als_opts", "evaluate", "quality_ybz", "foreground_eval", "foreground_scores", "report_scores", "triple_product", "unfold",
           "soft_threshold", "buildF", "buildG", "buildH", "Session", "Comm", "TritdError",
           "make_opts", "initial_factors", "PinvToleranceWarning"]
