"""CPU oracle of the held-out validation of the masked nonconvex solver
(holdout=) — TEST INFRASTRUCTURE ONLY.

The contract of include/tritd.h (tritd_ncvx_holdout_f64), restated.  Line
numbers are fast_robust_triple_tensor/test.m's.  With Omega the `observed` mask
(None = all true), H the `holdout` mask, patience >= 0 and val_norm in {2, 1}:

* only H & Omega counts: a flag outside Omega is ignored, whatever X holds there;
* the fit is tests/masked_ncvx_oracle.triple_decomp_ncvx_masked with
  Omega & ~H: with patience = 0 its A, B, C, O, errHist and k are that call's,
  bit for bit, and O is exactly 0 on H & Omega;
* with T_k = triple_product(A, B, C) of :35 in iteration k (the factors
  iteration k STARTED with),
    valHist(k)  = ||H o Omega o (X - T_k)|| / ||H o Omega o X||
    valHist1(k) = sum_{H & Omega} |X - T_k| / sum_{H & Omega} |X|,
  both truncated with errHist (:66);
* best_iter = the first minimum of the history val_norm picks (a strict <
  against the running best, k = 1 always taken); A_best, B_best, C_best are the
  factors iteration best_iter started with (best_iter = 1: A0, B0, C0);
* patience = p > 0: after the stop test of :65-68 for iteration k,
  k - best_iter >= p stops the loop at k like a reference break: the updates of
  k have run, O is that of k-1 (:71), both histories have k entries;
* stop_reason: 0 ran to maxIter, 1 the test of :65, 2 patience.

The loop itself is masked_ncvx_oracle's: it is run once with every iteration
traced (A, B, C and O_new after it), and the scores and the bookkeeping are
taken from the trace in iteration order.  T_k is recomputed from the factors
after iteration k-1 by the same triple_product, so it has the bits of :35.
Where patience stops the loop at k, the outputs are the traced factors of k,
the traced O_new of k-1 and errHist(1:k): what a break at k leaves.
"""
from __future__ import annotations

import numpy as np

import masked_ncvx_oracle as mno
import tritd_oracle as orc


def quiet(s):
    pass


def split_masks(X, observed, holdout):
    """(Omega & ~H, H & Omega) as column-major bool arrays of X's shape."""
    shape = orc.as3(X).shape
    W = np.ones(shape, dtype=bool) if observed is None else \
        (np.asarray(observed) != 0).reshape(shape, order="F")
    H = (np.asarray(holdout) != 0).reshape(shape, order="F")
    return np.asfortranarray(W & ~H), np.asfortranarray(H & W)


def scores(X, held, T):
    """(valHist, valHist1) of one T."""
    x = np.asarray(X)[held]
    d = x - np.asarray(T)[held]
    return (float(np.linalg.norm(d) / np.linalg.norm(x)),
            float(np.sum(np.abs(d)) / np.sum(np.abs(x))))


def triple_decomp_ncvx_holdout(X, observed, holdout, r, rho, lam, gamma_A, epsilon, p, theta,
                               maxIter, tol, A0, B0, C0, patience=0, val_norm=2):
    if holdout is None:
        raise ValueError("holdout is required")
    if patience < 0:
        raise ValueError("patience must be >= 0")
    if val_norm not in (1, 2):
        raise ValueError("val_norm must be 1 or 2")
    if rho == 0:
        raise ValueError("rho must be non-zero")
    fit, held = split_masks(X, observed, holdout)
    if not held.any():
        raise ValueError("holdout has no observed entry: nothing to score")
    if not fit.any():
        raise ValueError("no observed entry is left to fit beside the holdout")
    X = orc.as3(X)
    n1, n2, n3 = X.shape
    if np.linalg.norm(X[held]) == 0.0:
        raise ValueError("the held-out entries of X are all zero")
    maxIter = int(maxIter)
    run = mno.triple_decomp_ncvx_masked(X, fit, r, rho, lam, gamma_A, epsilon, p, theta, maxIter,
                                        tol, A0, B0, C0, printer=quiet,
                                        trace_iters=range(1, maxIter + 1))
    A, B, C, O, errHist, k_ref, trace = run
    start = {1: dict(A=orc.as3(A0).reshape((n1, r, r), order="F").copy(order="F"),
                     B=orc.as3(B0).reshape((r, n2, r), order="F").copy(order="F"),
                     C=orc.as3(C0).reshape((r, r, n3), order="F").copy(order="F"))}
    for it in range(2, k_ref + 1):
        start[it] = trace[it - 1]

    valHist, valHist1 = np.zeros(k_ref), np.zeros(k_ref)
    best, best_iter, k, stop_reason = np.inf, 0, k_ref, 0
    for it in range(1, k_ref + 1):                    # in the loop's order
        s = start[it]
        valHist[it - 1], valHist1[it - 1] = scores(X, held, orc.triple_product(s["A"], s["B"], s["C"]))
        v = valHist1[it - 1] if val_norm == 1 else valHist[it - 1]
        if it == 1 or v < best:
            best, best_iter = v, it
        if it == k_ref and it > 1 and \
                abs(errHist[it - 1] - errHist[it - 2]) < tol * errHist[it - 2]:
            stop_reason = 1                            # :65 broke the loop at k_ref
        elif patience > 0 and it - best_iter >= patience:
            k, stop_reason = it, 2
            break
    if stop_reason == 2:  # what a break at k leaves (:67 before :71)
        A, B, C = trace[k]["A"], trace[k]["B"], trace[k]["C"]
        O = trace[k - 1]["O"]
        errHist = errHist[:k]
    sb = start[best_iter]
    return dict(A=A, B=B, C=C, O=O, errHist=np.asarray(errHist)[:k], k=k, valHist=valHist[:k],
                valHist1=valHist1[:k], best_iter=best_iter, stop_reason=stop_reason,
                A_best=sb["A"], B_best=sb["B"], C_best=sb["C"], fit=fit, held_out=held)
