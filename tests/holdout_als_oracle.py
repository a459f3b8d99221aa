"""CPU oracle of the held-out validation error and early stopping of the masked
ALS (holdout=, patience=) — TEST INFRASTRUCTURE ONLY.

tests/masked_als_oracle.py restates fast_robust_triple_tensor/
triple_decomp_ALS.m:1-40 with an observation mask Omega.  This module restates
the contract of include/tritd.h (tritd_als_holdout_f64) on top of it, with
`tritd_oracle`'s functions.  H is a logical tensor of X's size; only
H & Omega counts.

* The fit is the masked ALS with observed = Omega & ~H, statement for
  statement: with patience = 0 the returned A, B, C, errHist, k are bit for
  bit those of ``masked_als_oracle.triple_decomp_ALS_masked`` with that mask.
* valHist(k) = ||H o Omega o (X - Xhat)|| / ||H o Omega o X|| with the Xhat of
  :15 in iteration k, truncated with errHist (:21).
* best_iter = argmin_k valHist(k), the first minimum (a strict < against the
  running best, k = 1 always taken); A_best, B_best, C_best are the factors
  iteration best_iter started with.
* patience = p > 0: after the stop test of :20, k - best_iter >= p stops the
  loop at k like a reference stop (the updates of k do not run).
* stop_reason: 0 ran to maxIter, 1 the test of :20, 2 patience.
"""
from __future__ import annotations

import numpy as np

import tritd_oracle as orc


def masks(X, observed, holdout):
    """(fit mask Omega & ~H, held-out set H & Omega), both of X's shape."""
    shape = orc.as3(X).shape
    W = np.ones(shape, dtype=bool) if observed is None else \
        (np.asarray(observed) != 0).reshape(shape, order="F")
    H = (np.asarray(holdout) != 0).reshape(shape, order="F") & W
    return W & ~H, H


def val_error(X, H, Xhat):
    """||H o (X - Xhat)|| / ||H o X|| over the entries of H (column-major order)."""
    h = H.ravel(order="F")
    x = np.asarray(X).ravel(order="F")[h]
    return float(np.linalg.norm(x - np.asarray(Xhat).ravel(order="F")[h]) / np.linalg.norm(x))


def triple_decomp_ALS_holdout(X, observed, holdout, r, opts, A0, B0, C0, patience=0, printer=None):
    """Returns ``(A, B, C, errHist, k, info)`` with info = dict(valHist,
    best_iter, stop_reason, A_best, B_best, C_best, holdout_count, decisions);
    decisions[k-2] = (valHist(k), running best before k) for k >= 2."""
    for f in ("maxIter", "tol"):
        if f not in opts:
            raise KeyError(f"Reference to non-existent field '{f}'.")
    maxIter = int(opts["maxIter"]); tol = float(opts["tol"])         # :2-3
    patience = int(patience)
    if patience < 0:
        raise ValueError("patience must be >= 0")
    X0 = orc.as3(X)
    n1, n2, n3 = X0.shape                                            # :5
    W, H = masks(X0, observed, holdout)
    if not H.any() or not W.any():
        raise ValueError("H & Omega and Omega & ~H must both be non-empty")
    Xh = np.where(H, X0, 0.0)                                        # H o Omega o X (fill values never enter)
    if np.linalg.norm(Xh.ravel(order="F")) == 0.0:
        raise ValueError("||H o Omega o X|| = 0")
    X = X0.copy(order="K")
    X[~W] = 0.0                                                      # X <- (Omega & ~H) o X
    Xnorm = np.linalg.norm(X.ravel(order="F"))                       # :6
    A = orc.as3(A0).reshape((n1, r, r), order="F").copy(order="F")  # :8
    B = orc.as3(B0).reshape((r, n2, r), order="F").copy(order="F")  # :9
    C = orc.as3(C0).reshape((r, r, n3), order="F").copy(order="F")  # :10
    errHist = np.zeros(max(maxIter, 0))                              # :12
    valHist = np.zeros(max(maxIter, 0))
    ridge = 1e-9 * np.eye(r * r)
    best, best_iter, stop_reason = np.inf, 0, 0
    Ab, Bb, Cb = A.copy(order="F"), B.copy(order="F"), C.copy(order="F")
    decisions = []
    k = 0

    def done():
        info = dict(valHist=valHist[:k], best_iter=best_iter, stop_reason=stop_reason, A_best=Ab,
                    B_best=Bb, C_best=Cb, holdout_count=int(H.sum()), decisions=decisions)
        return A, B, C, errHist[:k], k, info

    for k in range(1, maxIter + 1):                                  # :14
        Xhat = orc.triple_product(A, B, C)                            # :15
        Xt = X.copy(order="K")                                        # X~ = where(Omega & ~H, X, Xhat)
        Xt[~W] = Xhat[~W]
        errHist[k - 1] = np.linalg.norm(Xt.ravel(order="F") - Xhat.ravel(order="F")) / Xnorm  # :16
        valHist[k - 1] = val_error(Xh, H, Xhat)
        if k > 1:
            decisions.append((float(valHist[k - 1]), float(best)))
        if k == 1 or valHist[k - 1] < best:
            best, best_iter = valHist[k - 1], k
            Ab, Bb, Cb = A.copy(order="F"), B.copy(order="F"), C.copy(order="F")
        if k % 5 == 0:                                                # :17-19
            (printer or print)("Iteration %d, relative error = %.4e" % (k, errHist[k - 1]))
        if k > 1 and abs(errHist[k - 1] - errHist[k - 2]) < tol * errHist[k - 2]:  # :20
            stop_reason = 1
            return done()                                             # :21-22
        if patience > 0 and k - best_iter >= patience:
            stop_reason = 2
            return done()
        F = orc.buildF(B, C)                                          # :25-28 with X~
        A = orc.reshape_A_from_A1((orc.unfold(Xt, 1) @ F.T) @ orc.pinv(F @ F.T + ridge), n1, r)
        G = orc.buildG(A, C)                                          # :30-33 with X~
        B = orc.reshape_B_from_B2((orc.unfold(Xt, 2) @ G.T) @ orc.pinv(G @ G.T + ridge), n2, r)
        Hm = orc.buildH(A, B)                                         # :35-38 with X~
        C = orc.reshape_C_from_C3((orc.unfold(Xt, 3) @ Hm.T) @ orc.pinv(Hm @ Hm.T + ridge), n3, r)
    return done()
