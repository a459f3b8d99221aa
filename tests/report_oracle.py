"""CPU oracle of the video driver's report — TEST INFRASTRUCTURE ONLY.

A numpy restatement, statement for statement, of what
video_triple_comparison.m does with the solver's outputs (the line numbers on
the right), and of the raw parts tritd_session_report returns for it
(include/tritd.h).  The yardsticks are the oracle's `evaluate`,
`psnr_index` and `ssim_index` (oracle/tritd_oracle.py); `driver_figures` calls
them as the script does, `parts` states the sums they reduce to and
`figures_from_parts` the host arithmetic from those sums.
"""
import numpy as np

import tritd_oracle as orc

FIGURES = ("rmse", "nrmse", "srmse", "snrmse", "trmse", "tnrmse", "psnr", "ssim")


def driver_figures(X, missing, X_hat, O):
    """video_triple_comparison.m:36-37, :64-67 on X_hat = triple_product(A, B, C) (:56)."""
    X = np.asarray(X, dtype=np.float64)
    m = np.asarray(missing, dtype=bool)
    gt = X.ravel(order="F")[m.ravel(order="F")]                          # :36 gt = X(mask_missing)
    gt_2 = X.ravel(order="F")[~m.ravel(order="F")]                       # :37 gt_2 = X(~mask_missing)
    pick = lambda T, k: np.asarray(T).ravel(order="F")[k.ravel(order="F")]
    with np.errstate(divide="ignore", invalid="ignore"):                 # 0/0 = NaN, as in MATLAB
        rmse, nrmse = orc.evaluate(pick(X_hat, m), gt)                   # :64 evaluate(X_hat, gt, mask)
        srmse, snrmse = orc.evaluate(pick(O, ~m), gt_2)                  # :65 evaluate(O, gt_2, ~mask)
        trmse, tnrmse = orc.evaluate(np.asarray(X_hat) + np.asarray(O), X)   # :66
    n3 = X.shape[2]
    pf = np.array([orc.psnr_index(X[:, :, f], X_hat[:, :, f]) for f in range(n3)])   # :67 quality_ybz
    sf = np.array([orc.ssim_index(X[:, :, f], X_hat[:, :, f]) for f in range(n3)])
    return dict(rmse=float(rmse), nrmse=float(nrmse), srmse=float(srmse), snrmse=float(snrmse),
                trmse=float(trmse), tnrmse=float(tnrmse), psnr=float(np.mean(pf)),
                ssim=float(np.mean(sf)), psnr_frames=pf, ssim_frames=sf)


def parts(X, missing, L, O):
    """The raw parts of tritd_session_report: sums[6], frame_sq[n3], frame_ssim[n3].
    evaluate (:290-298): rmse = norm(X_hat(mask) - gt), nrmse = rmse / norm(gt), so
    rmse^2 and norm(gt)^2 are the sums below; psnr_index.m:4 divides 255^2 by
    mse(x - y) = frame_sq / (n1 n2)."""
    X = np.asarray(X, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    O = np.asarray(O, dtype=np.float64)
    m = np.zeros(X.shape, dtype=bool) if missing is None else np.asarray(missing, dtype=bool)
    sq = lambda v: float(np.dot(v.ravel(), v.ravel()))
    sums = np.array([sq((L - X)[m]), sq(X[m]),                           # :64
                     sq((O - X)[~m]), sq(X[~m]),                         # :65
                     sq((L + O) - X), sq(X)])                            # :66
    frame_sq = np.array([sq(L[:, :, f] - X[:, :, f]) for f in range(X.shape[2])])       # :67
    frame_ssim = np.array([orc.ssim_index(X[:, :, f], L[:, :, f]) for f in range(X.shape[2])])
    return dict(sums=sums, frame_sq=frame_sq, frame_ssim=frame_ssim)


def figures_from_parts(sums, frame_sq, frame_ssim, n1, n2):
    """The host arithmetic of tritd.report_scores, in the oracle's order of operations."""
    S = np.asarray(sums, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        root = np.sqrt(S)                                                # norm(.)
        out = dict(rmse=float(root[0]), nrmse=float(root[0] / root[1]),  # :294-295
                   srmse=float(root[2]), snrmse=float(root[2] / root[3]),
                   trmse=float(root[4]), tnrmse=float(root[4] / root[5]))
        pf = 10.0 * np.log10(255.0 ** 2 / (np.asarray(frame_sq, dtype=np.float64) / float(n1 * n2)))
    out.update(psnr=float(np.mean(pf)), psnr_frames=pf)                  # quality_ybz: mean over frames
    sf = np.asarray(frame_ssim, dtype=np.float64)
    out.update(ssim=float(np.mean(sf)), ssim_frames=sf)
    return out


# Tolerances, from the reference alone (tests/boundary_cases.py: rre_reference).
RTOL_SUM = 1e-12
TOL_TP = 1e-13


def tolerances(X, missing, L, O):
    """Relative tolerances of sums[6] and frame_sq[n3]: the denominators and S2
    (no product in them) take RTOL_SUM; a sum of (P - X)^2 with P = L or L + O
    moves by at most 2 TOL_TP |P| / |P - X| relative when the MFMA product
    moves by TOL_TP elementwise, the norms over the sum's own index set."""
    X = np.asarray(X, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    O = np.asarray(O, dtype=np.float64)
    m = np.zeros(X.shape, dtype=bool) if missing is None else np.asarray(missing, dtype=bool)
    nrm = lambda v: float(np.linalg.norm(np.asarray(v).ravel()))

    def moved(P, D):  # P and D = P - X over one index set
        return RTOL_SUM + 2.0 * TOL_TP * nrm(P) / nrm(D) if nrm(D) > 0 else RTOL_SUM

    sums = np.array([moved(L[m], (L - X)[m]), RTOL_SUM, RTOL_SUM, RTOL_SUM,
                     moved(L + O, (L + O) - X), RTOL_SUM])
    frames = np.array([moved(L[:, :, f], L[:, :, f] - X[:, :, f]) for f in range(X.shape[2])])
    return sums, frames


def ssim_sensitivity(X, L, rng):
    """The largest relative change of ssim_index(X(:,:,f), L(:,:,f)) over the
    frames when L is perturbed elementwise by +-TOL_TP (relative)."""
    X = np.asarray(X, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    Lp = L * (1.0 + TOL_TP * rng.choice([-1.0, 1.0], size=L.shape))
    worst = 0.0
    for f in range(X.shape[2]):
        a, b = orc.ssim_index(X[:, :, f], L[:, :, f]), orc.ssim_index(X[:, :, f], Lp[:, :, f])
        if np.isfinite(a) and a != 0.0:
            worst = max(worst, abs(b - a) / abs(a))
    return worst
