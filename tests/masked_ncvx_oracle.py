"""CPU oracle of the mask-aware nonconvex solver (observed=) — TEST
INFRASTRUCTURE ONLY.

`oracle/tritd_oracle.py` restates fast_robust_triple_tensor/test.m:1-73
(`triple_decomp_ADMM_ncvx`).  This module restates the same loop with an
observation mask Omega (a logical tensor of X's size, True = observed), using
that module's ncvx_update_A, ncvx_update_B, update_C, weighted_soft_threshold
and triple_product.  Everything not mentioned below is the reference's
statement, in the reference's expression order:

* before the loop  X <- Omega o X (unobserved entries set to 0, so their fill
  values, NaN and Inf included, never enter) and Xnorm = ||Omega o X|| (:21);
* in iteration k, after T = triple_product(A,B,C) (:35),
  X~ = where(Omega, X, T) stands for X in :36, :44, :47, :48, :62 and in the
  three factor updates :49-51;
* at an unobserved entry the exact-arithmetic values of :36-48 for x = T,
  O = Lambda = Gamma = 0 are imposed, not computed: Y_new = T, O_new = 0,
  Lambda and Gamma keep their value (so both stay exactly 0), and the entry
  adds exactly 0 to errHist(k).  (In floating point (T + rho T)/(1 + rho) is
  not T: left to rounding it would leak 1e-16-sized residue into Gamma and
  errHist, and O would be nonzero at missing entries when lambda = 0.)

Unchanged: the stop test (:65-68), the truncation of errHist, the returned O
being that of iteration k-1 on a break (:71) and the progress line of every
iteration (:63).  With Omega all true every statement is the reference's, bit
for bit (tests/test_masked_ncvx_oracle.py).
"""
from __future__ import annotations

import numpy as np

import tritd_oracle as orc


def triple_decomp_ncvx_masked(X, observed, r, rho, lam, gamma_A, epsilon, p, theta, maxIter, tol,
                              A0, B0, C0, printer=None, trace_iters=()):
    """Returns ``(A, B, C, O, errHist, k, trace)`` like
    ``tritd_oracle.triple_decomp_ADMM_ncvx``; ``observed=None`` means all
    true.  ``trace[k]`` holds A, B, C, O (= O_new), Lam, Gam after iteration k."""
    X = orc.as3(X)
    n1, n2, n3 = X.shape                                              # :20
    W = np.ones(X.shape, dtype=bool) if observed is None else \
        (np.asarray(observed) != 0).reshape(X.shape, order="F")
    U = ~W
    X = X.copy(order="F")
    X[U] = 0.0                                                        # X <- Omega o X
    Xnorm = np.linalg.norm(X.ravel(order="F"))                        # :21 over the observed entries
    A = orc.as3(A0).reshape((n1, r, r), order="F").copy(order="F")   # :24-26
    B = orc.as3(B0).reshape((r, n2, r), order="F").copy(order="F")
    C = orc.as3(C0).reshape((r, r, n3), order="F").copy(order="F")
    O = np.zeros((n1, n2, n3), order="F")                             # :28
    Lam = np.zeros((n1, n2, n3), order="F")                           # :29
    Gam = np.zeros((n1, n2, n3), order="F")                           # :30
    errHist = np.zeros(int(maxIter))                                  # :32
    trace = {}
    k = 0
    for k in range(1, int(maxIter) + 1):                              # :34
        T = orc.triple_product(A, B, C)                               # :35
        Xt = X.copy(order="F")                                        # X~ = where(Omega, X, T)
        Xt[U] = T[U]
        Y_new = ((Xt - O) + rho * (T + Lam / rho)) / (1 + rho)        # :36
        Y_new[U] = T[U]                                               # imposed
        W_O = np.ones(O.shape)                                        # :43
        O_new = orc.weighted_soft_threshold((Xt - Y_new) + Gam / rho, lam / rho, W_O)   # :44
        O_new[U] = 0.0                                                # imposed
        dLam = T - Y_new                                              # exactly 0 where unobserved
        Lam = Lam + rho * dLam                                        # :47
        res = (Xt - Y_new) - O_new                                    # exactly 0 where unobserved
        Gam = Gam + rho * res                                         # :48
        A = orc.ncvx_update_A(Xt, A, B, C, gamma_A, epsilon, p, theta)   # :49 with X~
        B = orc.ncvx_update_B(Xt, A, B, C)                            # :50 with X~
        C = orc.update_C(Xt, A, B, C)                                 # :51 with X~
        errHist[k - 1] = np.linalg.norm(res.ravel(order="F")) / Xnorm    # :62
        (printer or print)("Iteration %d, relative error = %.4e" % (k, errHist[k - 1]))  # :63
        if k in trace_iters:
            trace[k] = dict(A=A.copy(order="F"), B=B.copy(order="F"), C=C.copy(order="F"),
                            O=O_new.copy(order="F"), Lam=Lam.copy(order="F"),
                            Gam=Gam.copy(order="F"))
        if k > 1 and abs(errHist[k - 1] - errHist[k - 2]) < tol * errHist[k - 2]:  # :65
            errHist = errHist[:k]                                     # :66
            break                                                     # :67 (O keeps iteration k-1)
        O = O_new                                                     # :71
    return A, B, C, O, errHist, k, trace


def missing_error(A, B, C, truth, observed):
    """Relative error of triple_product(A,B,C) on the unobserved entries."""
    miss = ~np.asarray(observed, dtype=bool)
    L = orc.triple_product(A, B, C)
    return float(np.linalg.norm((L - truth)[miss]) / np.linalg.norm(np.asarray(truth)[miss]))
