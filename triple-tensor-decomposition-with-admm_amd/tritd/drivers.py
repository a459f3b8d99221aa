"""Driver-side data path of the reference experiments.

The TRIPLE branches of the two driver scripts, on the GPU path:

    traffic_triple(X, ...)   traffic_triple_comparison.m:20-64   (completion, RRE)
    video_triple(X, ...)     video_triple_comparison.m:19-76     (background
                             separation: RMSE/NRMSE on the missing and observed
                             entries, total RRE, PSNR/SSIM of the low-rank part)
    load_dataset(path)       the `load(name + ".mat")` of both scripts (:20 / :20)

The solver, `triple_product`, `evaluate` and `quality_ybz` all run through
libtritd.so; only the mask draw, the `Y(mask) = 0` copy and the `X_hat + O`
sum are host numpy (the reference does them in MATLAB on the host too).
MATLAB's `randperm` stream cannot be reproduced, so the missing-entry mask
comes from a seeded numpy generator (same count, `round(ratio * numel)`).
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import api

# traffic_triple_comparison.m:42-50 / video_triple_comparison.m:41-49
TRAFFIC_OPTS = dict(maxIter=100, tol=1e-5, mu=1e-3, **{"lambda": 1.8}, lambda2=1e-3, rho=1.25,
                    alphaA=1e-3, alphaB=1e-3, disp=1)
VIDEO_OPTS = dict(maxIter=100, tol=1e-5, mu=1e-2, **{"lambda": 1.8}, lambda2=1e-2, rho=1.2,
                  alphaA=1e-3, alphaB=1e-3, disp=1)


def load_dataset(path, kind="traffic"):
    """`load(name + ".mat")`: the traffic script reads variable T
    (traffic_triple_comparison.m:20-22, `X = double(T)`, taxi cut to 500
    slices at :23-25), the video script `gray_images` (video_triple_comparison.m:20-21).
    MAT v5/v7 files through scipy.io; a v7.3 (HDF5) file is refused with a
    message (h5py is not available here)."""
    from scipy.io import loadmat
    try:
        m = loadmat(path)
    except NotImplementedError as e:  # v7.3
        raise ValueError(f"{path}: MAT v7.3 (HDF5) files need h5py, which is not installed") from e
    var = "T" if kind == "traffic" else "gray_images"
    if var not in m:
        raise KeyError(f"{path}: variable '{var}' not found (have {sorted(k for k in m if not k.startswith('__'))})")
    X = np.asfortranarray(np.asarray(m[var], dtype=np.float64))
    if kind == "traffic" and os.path.basename(path).startswith("taxi"):
        X = np.asfortranarray(X[:, :, :500])
    return X


def missing_mask(shape, ratio, rng):
    """Step 1 of both scripts: `num_to_zero = round(ratio*numel)` distinct
    positions drawn uniformly (randperm), returned as a logical array."""
    total = int(np.prod(shape))
    num = int(np.floor(ratio * total + 0.5))  # MATLAB round (half away from zero, ratio >= 0)
    idx = rng.permutation(total)[:num]
    mask = np.zeros(total, dtype=bool)
    mask[idx] = True
    return mask.reshape(shape, order="F")


def _observe(X, mask, fill=0.0):
    Y = np.array(X, dtype=np.float64, order="F", copy=True)
    Y[mask] = fill
    return Y


def _mask_args(use_mask, mask):
    """use_mask -> (the fill of the missing entries, the solver's `observed`):
    False: zeros and no mask (the reference); True: zeros and `~mask`; "nan":
    NaN at the missing entries and observed="nan" (the mask is then derived
    from the data on the device)."""
    if isinstance(use_mask, str):
        if use_mask != "nan":
            raise ValueError('use_mask must be False, True or "nan", got %r' % (use_mask,))
        return np.nan, "nan"
    return 0.0, (~mask if use_mask else None)


def traffic_triple(X, r=5, missing_ratio=0.15, *, opts=None, seed=0, A0=None, B0=None, C0=None,
                   printer=print, name="data", use_mask=False):
    """TRIPLE branch of traffic_triple_comparison.m (:26-64): mask, zero the
    missing entries, solve, `X_hat = triple_product(A,B,C)`, RRE over all
    entries with `evaluate(X_hat, X, true(size(X)))`, print as at :64.
    `use_mask` (not in the reference, which lets the solver explain the zeros
    as outliers) tells the solver which entries are missing
    (`observed = ~mask`): it then fits the observed ones only.
    `use_mask="nan"` writes NaN at the missing entries instead of zeros and
    passes `observed="nan"`: the same fit, with no mask array made or uploaded."""
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    rng = np.random.default_rng(seed)
    mask = missing_mask(X.shape, missing_ratio, rng)
    printer("\n===== Dataset: %s Missing Radio %.3f=====" % (name, missing_ratio))
    fill, observed = _mask_args(use_mask, mask)
    Y = _observe(X, mask, fill)
    o = dict(TRAFFIC_OPTS if opts is None else opts)
    t0 = time.perf_counter()
    A, B, C, O, errHist = api.triple_decomp_ADMM(Y, r, o, A0, B0, C0, observed=observed)
    timer = time.perf_counter() - t0
    X_hat = api.triple_product(A, B, C)
    rmse, nrmse = api.evaluate(X_hat, X)
    printer("TRIPLE ADMM - RRE: %.2f, Time: %.2f s" % (nrmse, timer))
    return dict(A=A, B=B, C=C, O=O, errHist=errHist, X_hat=X_hat, mask=mask, rmse=rmse,
                nrmse=nrmse, time=timer)


def video_triple(X, r=5, missing_ratio=0.0, *, opts=None, seed=0, A0=None, B0=None, C0=None,
                 printer=print, name="data", save_dir=None, use_mask=False, groundtruth=None,
                 thr=50.0, session=False):
    """TRIPLE branch of video_triple_comparison.m (:26-76) through the
    `triple_decomp_ADMM_outlier` name the script calls (:54): RMSE/NRMSE of
    X_hat on the missing entries, of O on the observed ones, of X_hat + O on
    all of them, and PSNR/SSIM of X_hat against X (quality_ybz), printed as at
    :74-75.  With `save_dir` the observed tensor is saved as `<name>_raw.mat`
    (variable Y, :32, every ratio) and, when missing_ratio == plot_rate == 0
    (:58), the errHist / X_hat / O .mat files of :59-61.  `use_mask` passes
    `observed = ~mask` to the solver, `use_mask="nan"` NaN-marked data and
    `observed="nan"` (see traffic_triple).

    `groundtruth` (CDnet labels of X's shape: 255 = motion, 170 = unknown) adds
    the script's `eval` (:316-371) on the returned O with the threshold `thr`
    (the reference's 50, :339): its five lines (:366-370) are printed after the
    line above and the result gains `precision, recall, f1, pwc, fg_counts`
    (per frame: TP, FP, FN, TN) and `fg_mask`.  Without it nothing changes.

    `session=True` solves through a `Session` and takes the eight figures from
    `Session.report` (and, with `groundtruth`, the foreground scores from
    `Session.foreground`) while the tensors are still on the device: X_hat and
    O are downloaded only for the returned dict and the .mat files.  The same
    lines are printed in the same format.  With the default nothing changes."""
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    rng = np.random.default_rng(seed)
    mask = missing_mask(X.shape, missing_ratio, rng)
    printer("\n===== Dataset: %s Missing Radio %.3f=====" % (name, missing_ratio))
    fill, observed = _mask_args(use_mask, mask)
    Y = _observe(X, mask, fill)
    if save_dir is not None:  # save(sprintf("%s_raw.mat", name), 'Y')  (:32)
        from scipy.io import savemat
        savemat(os.path.join(save_dir, "%s_raw.mat" % name), {"Y": Y})
    gt = X.ravel(order="F")[mask.ravel(order="F")]       # X(mask_missing), column-major (:36)
    gt_2 = X.ravel(order="F")[~mask.ravel(order="F")]    # X(~mask_missing)              (:37)
    o = dict(VIDEO_OPTS if opts is None else opts)
    if session:
        return _video_triple_session(X, Y, mask, r, o, A0, B0, C0, observed if use_mask else None,
                                     printer, name, save_dir, missing_ratio, groundtruth, thr)
    t0 = time.perf_counter()
    A, B, C, O, errHist = api.triple_decomp_ADMM_outlier(Y, r, o, A0, B0, C0,
                                                         **(dict(observed=observed) if use_mask else {}))
    timer = time.perf_counter() - t0
    X_hat = api.triple_product(A, B, C)
    if save_dir is not None and missing_ratio == 0:
        from scipy.io import savemat
        savemat(os.path.join(save_dir, "%s_triple_re_errHist.mat" % name), {"errHist": errHist})
        savemat(os.path.join(save_dir, "%s_triple_re_Xhat.mat" % name), {"X_hat_re": X_hat})
        savemat(os.path.join(save_dir, "%s_triple_re_O.mat" % name), {"O": O})
    # with no missing entries gt is empty: norm([]) = 0 and nrmse = 0/0 = NaN, as in MATLAB
    rmse, nrmse = api.evaluate(X_hat, gt, mask)
    rmse2, nrmse2 = api.evaluate(O, gt_2, ~mask)
    rmse3, nrmse3 = api.evaluate(np.asfortranarray(X_hat + O), X)
    psnr, ssim = api.quality_ybz(X, X_hat)
    printer(_VIDEO_LINE % (rmse, nrmse, rmse2, nrmse2, rmse3, nrmse3, psnr, ssim, timer))
    out = dict(A=A, B=B, C=C, O=O, errHist=errHist, X_hat=X_hat, mask=mask, rmse=rmse,
               nrmse=nrmse, srmse=rmse2, snrmse=nrmse2, trmse=rmse3, tnrmse=nrmse3, psnr=psnr,
               ssim=ssim, time=timer)
    if groundtruth is not None:  # eval(X, groundtruth, X_hat, O)  (:316-371)
        _print_foreground(api.foreground_eval(O, groundtruth, thr), printer, out)
    return out


_VIDEO_LINE = ("TRIPLE ADMM - RMSE: %.4e, NRMSE: %.4e, SRMSE: %.4e, SNRMSE: %.4e, TRMSE: %.4e, "
               "TNRMSE: %.4e, PSNR: %.4e, SSIM: %.4e, Time: %.2f s")


def _print_foreground(fg, printer, out):
    TP, FP, FN, TN = (int(v) for v in fg["total"])
    printer("TP: %d FP: %d TN: %d FN: %d " % (TP, FP, TN, FN))   # :366
    printer("Precision: %.4f" % fg["precision"])                 # :367
    printer("Recall   : %.4f" % fg["recall"])                    # :368
    printer("F1 Score : %.4f" % fg["f1"])                        # :369
    printer("PWC      : %.4f%%" % fg["pwc"])                     # :370
    out.update(precision=fg["precision"], recall=fg["recall"], f1=fg["f1"], pwc=fg["pwc"],
               fg_counts=fg["counts"], fg_mask=fg["mask"])


def _video_triple_session(X, Y, mask, r, o, A0, B0, C0, observed, printer, name, save_dir,
                          missing_ratio, groundtruth, thr):
    """video_triple(session=True): the solve of :54 as a Session run to
    maxIter, the figures of :64-67 from Session.report and eval (:316-371)
    from Session.foreground, on the device; then the downloads for the caller."""
    n1, n2, n3 = X.shape
    start = dict(A0=A0, B0=B0, C0=C0) if all(a is not None for a in (A0, B0, C0)) else o
    A0, B0, C0 = api.initial_factors(n1, n2, n3, int(r), start)
    t0 = time.perf_counter()
    s = api.Session(int(r), o, A0, B0, C0, n1=n1, n2=n2, n3=n3, D=Y, probe=False,
                    observed=observed)
    try:
        s.run(s.maxIter)
        s.sync()
        timer = time.perf_counter() - t0
        # with no missing entries S0 = S1 = 0: rmse 0 and nrmse = 0/0 = NaN, as in MATLAB
        rep = s.report(X, mask if mask.any() else None)
        fg = s.foreground(thr, groundtruth) if groundtruth is not None else None
        g = s.get()
    finally:
        s.close()
    A, B, C, O, errHist = g["A"], g["B"], g["C"], g["O"], g["errHist"]
    X_hat = api.triple_product(A, B, C)
    if save_dir is not None and missing_ratio == 0:
        from scipy.io import savemat
        savemat(os.path.join(save_dir, "%s_triple_re_errHist.mat" % name), {"errHist": errHist})
        savemat(os.path.join(save_dir, "%s_triple_re_Xhat.mat" % name), {"X_hat_re": X_hat})
        savemat(os.path.join(save_dir, "%s_triple_re_O.mat" % name), {"O": O})
    figures = tuple(rep[k] for k in ("rmse", "nrmse", "srmse", "snrmse", "trmse", "tnrmse", "psnr",
                                     "ssim"))
    printer(_VIDEO_LINE % (figures + (timer,)))
    out = dict(A=A, B=B, C=C, O=O, errHist=errHist, X_hat=X_hat, mask=mask, time=timer,
               **{k: rep[k] for k in ("rmse", "nrmse", "srmse", "snrmse", "trmse", "tnrmse", "psnr",
                                      "ssim")})
    if fg is not None:
        _print_foreground(fg, printer, out)
    return out


def holdout_mask(observed, ratio, rng):
    """H: `round(ratio * nnz(observed))` of the observed entries, drawn like
    `missing_mask` (a permutation of their column-major positions)."""
    obs = np.asarray(observed, dtype=bool)
    idx = np.flatnonzero(obs.ravel(order="F"))
    num = int(np.floor(ratio * idx.size + 0.5))
    H = np.zeros(obs.size, dtype=bool)
    H[idx[rng.permutation(idx.size)[:num]]] = True
    return np.asfortranarray(H.reshape(obs.shape, order="F"))


def select_rank(X, observed, ranks, holdout_ratio=0.15, opts=None, seed=0, patience=0, *,
                factors=None, device=-1, solver=None, lambdas=None, val_norm=2, gammas=None):
    """Choose r by held-out validation (not in the reference): H is drawn from
    the observed entries with a seeded generator, every candidate rank is
    solved by `triple_decomp_ALS(observed=, holdout=H, patience=)`, and the
    rank whose minimum valHist is smallest wins (the first on a tie).

    `observed=None` means every entry, `observed="nan"` the entries of X that
    are not NaN (the solver then takes its mask from X too).  `factors(r)` returns (A0, B0, C0) for a
    rank (default: drawn by the solver).  Returns dict(rank=, holdout=H,
    results={r: dict(min_val=, best_iter=, stop_reason=, k=, A=, B=, C=,
    valHist=, errHist=)}) with A, B, C the best iterate's factors.

    `solver` is None or "als" (the above), a callable with
    `triple_decomp_ALS`'s signature, or "admm": the robust ADMM
    (`triple_decomp_ADMM(observed=, holdout=H, patience=, val_norm=)`, `opts`
    its options) over `ranks` x `lambdas` (default: the lambda of `opts`).
    The pair whose minimum of the chosen history (`val_norm`: 2 valHist,
    1 valHist1) is smallest wins, the first on a tie; nothing is solved again.
    The result then also has `lam=`, `results` is keyed by (r, lambda) and its
    entries also hold `valHist1` and `lam`.

    `solver="ncvx"` is the nonconvex solver of test.m
    (`triple_decomp_ncvx(observed=, holdout=H, patience=, val_norm=)`): `opts`
    holds its parameters `rho, lam, gamma_A, epsilon, p, theta, maxIter, tol`,
    and the grid is `ranks` x `lambdas` x `gammas` (defaults: the `lam` and the
    `gamma_A` of `opts`).  It is otherwise like "admm": the result also has
    `lam=` and `gamma_A=`, and `results` is keyed by (r, lambda, gamma_A)."""
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    if isinstance(observed, str):  # "nan": H needs the positions, the solver derives its own mask
        api._check_observed(observed)
        obs, obs_arg = ~np.isnan(X), observed
    else:
        obs = np.ones(X.shape, dtype=bool) if observed is None else np.asarray(observed) != 0
        obs_arg = obs
    H = holdout_mask(obs, holdout_ratio, np.random.default_rng(seed))
    if isinstance(solver, str) and solver not in ("als", "admm", "ncvx"):
        raise ValueError("solver must be 'als', 'admm', 'ncvx' or a callable")
    if solver == "ncvx":
        if opts is None:
            raise ValueError("solver='ncvx' needs the nonconvex parameters")
        names = ("rho", "lam", "gamma_A", "epsilon", "p", "theta", "maxIter", "tol")
        missing = [n for n in names if api._get(opts, n) is None]
        if missing:
            raise ValueError("solver='ncvx': opts lacks %s" % ", ".join(missing))
        prm = {n: api._get(opts, n) for n in names}
        lams = [prm["lam"]] if lambdas is None else list(lambdas)
        gams = [prm["gamma_A"]] if gammas is None else list(gammas)
        hist = "valHist1" if val_norm == 1 else "valHist"
        results, chosen = {}, None
        for r in ranks:
            A0, B0, C0 = factors(r) if factors is not None else (None, None, None)
            for lam in lams:
                for gam in gams:
                    _, _, _, _, errHist, k, v = api.triple_decomp_ncvx(
                        X, r, prm["rho"], lam, gam, prm["epsilon"], prm["p"], prm["theta"],
                        prm["maxIter"], prm["tol"], A0, B0, C0, device=device, return_iters=True,
                        observed=obs_arg, holdout=H, patience=patience, val_norm=val_norm)
                    key = (r, lam, gam)
                    results[key] = dict(
                        min_val=float(v[hist][v["best_iter"] - 1]), best_iter=v["best_iter"],
                        stop_reason=v["stop_reason"], k=k, A=v["A_best"], B=v["B_best"],
                        C=v["C_best"], valHist=v["valHist"], valHist1=v["valHist1"],
                        errHist=errHist, lam=lam, gamma_A=gam)
                    if chosen is None or results[key]["min_val"] < results[chosen]["min_val"]:
                        chosen = key
        return dict(rank=chosen[0], lam=chosen[1], gamma_A=chosen[2], holdout=H, results=results)
    if solver == "admm":
        if opts is None:
            raise ValueError("solver='admm' needs the ADMM opts")
        lams = [api._get(opts, "lambda")] if lambdas is None else list(lambdas)
        hist = "valHist1" if val_norm == 1 else "valHist"
        results, chosen = {}, None
        for r in ranks:
            A0, B0, C0 = factors(r) if factors is not None else (None, None, None)
            for lam in lams:
                o = dict(opts)
                o["lambda"] = lam
                _, _, _, _, errHist, k, v = api.triple_decomp_ADMM(
                    X, r, o, A0, B0, C0, device=device, return_iters=True, observed=obs_arg,
                    holdout=H, patience=patience, val_norm=val_norm)
                results[(r, lam)] = dict(
                    min_val=float(v[hist][v["best_iter"] - 1]), best_iter=v["best_iter"],
                    stop_reason=v["stop_reason"], k=k, A=v["A_best"], B=v["B_best"], C=v["C_best"],
                    valHist=v["valHist"], valHist1=v["valHist1"], errHist=errHist, lam=lam)
                if chosen is None or results[(r, lam)]["min_val"] < results[chosen]["min_val"]:
                    chosen = (r, lam)
        return dict(rank=chosen[0], lam=chosen[1], holdout=H, results=results)
    o = dict(maxIter=100, tol=1e-5) if opts is None else opts
    solve = api.triple_decomp_ALS if solver is None or solver == "als" else solver
    results, chosen = {}, None
    for r in ranks:
        A0, B0, C0 = factors(r) if factors is not None else (None, None, None)
        _, _, _, errHist, k, v = solve(X, r, o, A0, B0, C0, device=device, return_iters=True,
                                       observed=obs_arg, holdout=H, patience=patience)
        results[r] = dict(min_val=float(v["valHist"][v["best_iter"] - 1]), best_iter=v["best_iter"],
                          stop_reason=v["stop_reason"], k=k, A=v["A_best"], B=v["B_best"],
                          C=v["C_best"], valHist=v["valHist"], errHist=errHist)
        if chosen is None or results[r]["min_val"] < results[chosen]["min_val"]:
            chosen = r
    return dict(rank=chosen, holdout=H, results=results)
