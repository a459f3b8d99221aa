"""CPU oracle of the mask-aware ALS (observed=) — TEST INFRASTRUCTURE ONLY.

`oracle/tritd_oracle.py` restates fast_robust_triple_tensor/triple_decomp_ALS.m
:1-40.  This module restates the same loop with an observation mask Omega (a
logical tensor of X's size, True = observed), using that module's buildF/G/H,
unfold, pinv, reshape_* and triple_product.  Everything not mentioned below
is the reference's statement, in the reference's expression order:

* before the loop  X <- Omega o X (unobserved entries set to 0, so their fill
  values, NaN and Inf included, never enter) and Xnorm = ||Omega o X|| (:6);
* in iteration k, after Xhat = triple_product(A,B,C) (:15),
  X~ = where(Omega, X, Xhat) stands for X in :16 and in all three updates of
  that iteration (:25-38).

Consequences (checked by tests/test_masked_als_oracle.py): X~ - Xhat is exactly
0 at an unobserved entry, so errHist counts observed entries only; the
updates impute the missing data with the model of the iteration's start (EM
for the masked least-squares fit, so errHist never increases); with Omega all
true every statement is the reference's, bit for bit.
"""
from __future__ import annotations

import numpy as np

import tritd_oracle as orc


def triple_decomp_ALS_masked(X, observed, r, opts, A0, B0, C0, printer=None):
    """Returns ``(A, B, C, errHist, k)`` like ``tritd_oracle.triple_decomp_ALS``;
    ``observed=None`` means all true."""
    for f in ("maxIter", "tol"):
        if f not in opts:
            raise KeyError(f"Reference to non-existent field '{f}'.")
    maxIter = int(opts["maxIter"]); tol = float(opts["tol"])         # :2-3
    X = orc.as3(X)
    n1, n2, n3 = X.shape                                             # :5
    W = np.ones(X.shape, dtype=bool) if observed is None else \
        (np.asarray(observed) != 0).reshape(X.shape, order="F")
    X = X.copy(order="K")                                            # (X's own memory order)
    X[~W] = 0.0                                                      # X <- Omega o X
    Xnorm = np.linalg.norm(X.ravel(order="F"))                       # :6 over the observed entries
    A = orc.as3(A0).reshape((n1, r, r), order="F").copy(order="F")  # :8
    B = orc.as3(B0).reshape((r, n2, r), order="F").copy(order="F")  # :9
    C = orc.as3(C0).reshape((r, r, n3), order="F").copy(order="F")  # :10
    errHist = np.zeros(max(maxIter, 0))                              # :12
    ridge = 1e-9 * np.eye(r * r)
    k = 0
    for k in range(1, maxIter + 1):                                  # :14
        Xhat = orc.triple_product(A, B, C)                            # :15
        Xt = X.copy(order="K")                                        # X~ = where(Omega, X, Xhat)
        Xt[~W] = Xhat[~W]
        errHist[k - 1] = np.linalg.norm(Xt.ravel(order="F") - Xhat.ravel(order="F")) / Xnorm  # :16
        if k % 5 == 0:                                                # :17-19
            (printer or print)("Iteration %d, relative error = %.4e" % (k, errHist[k - 1]))
        if k > 1 and abs(errHist[k - 1] - errHist[k - 2]) < tol * errHist[k - 2]:  # :20
            errHist = errHist[:k]                                     # :21
            return A, B, C, errHist, k                                # :22
        F = orc.buildF(B, C)                                          # :25-28 with X~
        A = orc.reshape_A_from_A1((orc.unfold(Xt, 1) @ F.T) @ orc.pinv(F @ F.T + ridge), n1, r)
        G = orc.buildG(A, C)                                          # :30-33 with X~
        B = orc.reshape_B_from_B2((orc.unfold(Xt, 2) @ G.T) @ orc.pinv(G @ G.T + ridge), n2, r)
        H = orc.buildH(A, B)                                          # :35-38 with X~
        C = orc.reshape_C_from_C3((orc.unfold(Xt, 3) @ H.T) @ orc.pinv(H @ H.T + ridge), n3, r)
    return A, B, C, errHist, k


def missing_error(A, B, C, truth, observed):
    """Relative error of triple_product(A,B,C) on the unobserved entries."""
    miss = ~np.asarray(observed, dtype=bool)
    L = orc.triple_product(A, B, C)
    return float(np.linalg.norm((L - truth)[miss]) / np.linalg.norm(np.asarray(truth)[miss]))
