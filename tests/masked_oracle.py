"""CPU oracle of the mask-aware ADMM (opts.observed) — TEST INFRASTRUCTURE ONLY.

`oracle/tritd_oracle.py` restates triple_decomp_ADMM.m:15-68.  This module
restates the same loop with an observation mask Omega (a logical tensor of
D's size, True = observed), using that module's update_A/B/C, triple_product
and MATLAB helpers.  Everything not mentioned below is the reference's
statement, in the reference's expression order:

* before the loop  D <- Omega o D (unobserved entries set to 0, so their fill
  values, NaN included, never enter) and normD = ||Omega o D||;
* in each iteration, after L = triple_product(A,B,C) (:38),
  D~ = where(Omega, D, L) stands for D in :41 and :50, and in the next
  iteration's T = D~ - O + Y_L/mu (:33); for iteration 1, D~ = Omega o D.

Consequences (checked by tests/test_masked_oracle.py): D~ - L is exactly 0 at
an unobserved entry, so O, E, Y_L and Y_O stay exactly 0 there for every k;
T = L^(k-1) there, i.e. the factor update imputes the missing data with the
current model (EM / majorisation of the masked least-squares fit); errHist
counts observed entries only; with Omega all true every statement is the
reference's, bit for bit.
"""
from __future__ import annotations

import numpy as np

import tritd_oracle as orc


def triple_decomp_ADMM_masked(D, observed, r, opts, A0, B0, C0, trace_iters=()):
    """Returns ``(A, B, C, O, errHist, E, k, trace)`` like
    ``tritd_oracle.triple_decomp_ADMM``; ``observed=None`` means all true."""
    orc.check_opts(opts)
    D = orc.as3(D)
    n1, n2, n3 = D.shape
    W = np.ones(D.shape, dtype=bool) if observed is None else \
        (np.asarray(observed) != 0).reshape(D.shape, order="F")
    muL = float(opts["mu"]); rhoL = float(opts["rho"]); muL_max = float(opts["mu"]) * 1e6   # :16
    muO = float(opts["mu"]); rhoO = float(opts["rho"]); muO_max = float(opts["mu"]) * 1e6   # :17
    lam = float(opts["lambda"])                                      # :18
    lambda2 = float(opts["lambda2"])                                 # :19
    maxIter = int(opts["maxIter"]); tol = float(opts["tol"])         # :20
    model = orc.opts_model(opts)

    A = orc.as3(A0).reshape((n1, r, r), order="F").copy(order="F")  # :23
    B = orc.as3(B0).reshape((r, n2, r), order="F").copy(order="F")
    C = orc.as3(C0).reshape((r, r, n3), order="F").copy(order="F")
    O = np.zeros((n1, n2, n3), order="F"); E = O.copy(order="F")    # :24
    Y_L = np.zeros((n1, n2, n3), order="F")                          # :25
    Y_O = np.zeros((n1, n2, n3), order="F")                          # :26

    D = D.copy(order="K")                                            # (D's own memory order)
    D[~W] = 0.0                                                      # D <- Omega o D
    normD = np.linalg.norm(D.ravel(order="F"))                       # :28 over the observed entries
    errHist = np.zeros(maxIter)                                      # :29
    trace = {}
    Dt = D                                                           # D~ of iteration 1

    k = 0
    for k in range(1, maxIter + 1):                                  # :31
        T = (Dt - O) + (1.0 / muL) * Y_L                              # :33 with D~
        A = orc.update_A(T, A, B, C, lambda2, model)                  # :34
        B = orc.update_B(T, A, B, C, lambda2, model)                  # :35
        C = orc.update_C(T, A, B, C, model)                           # :36

        L = orc.triple_product(A, B, C, model)                        # :38
        Dt = D.copy(order="K")                                        # D~ = where(Omega, D, L)
        Dt[~W] = L[~W]

        R1 = (Dt - L) + (1.0 / muL) * Y_L                             # :41 with D~
        R2 = E - (1.0 / muO) * Y_O                                    # :42
        O = (muL * R1 + muO * R2) / (muL + muO)                       # :43

        R3 = O + (1.0 / muO) * Y_O                                    # :46
        E = orc.matlab_sign(R3) * orc.matlab_max0(np.abs(R3) - lam / muO)  # :47

        resL = (Dt - L) - O                                           # :50 with D~
        resO = O - E                                                  # :51
        Y_L = Y_L + muL * resL                                        # :52
        Y_O = Y_O + muO * resO                                        # :53

        muL = min(muL * rhoL, muL_max)                                # :56
        muO = min(muO * rhoO, muO_max)                                # :57

        errL = np.linalg.norm(resL.ravel(order="F")) / normD
        errO = np.linalg.norm(resO.ravel(order="F")) / normD
        errHist[k - 1] = errL + errO                                  # :59
        if k in trace_iters:
            trace[k] = dict(A=A.copy(order="F"), B=B.copy(order="F"), C=C.copy(order="F"),
                            O=O.copy(order="F"), E=E.copy(order="F"),
                            Y_L=Y_L.copy(order="F"), Y_O=Y_O.copy(order="F"), L=L.copy(order="F"))
        if k > 1 and abs(errHist[k - 1] - errHist[k - 2]) < tol * errHist[k - 2]:  # :63
            break

    errHist = errHist[:k]                                             # :68
    return A, B, C, O, errHist, E, k, trace


def rre(L, X):
    """Driver RRE (traffic_triple_comparison.m:62-63,194-199) over all entries."""
    return float(np.linalg.norm((L - X).ravel()) / np.linalg.norm(np.asarray(X).ravel()))
