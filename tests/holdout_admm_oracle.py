"""CPU oracle of the held-out validation of the masked ADMM (holdout=) — TEST
INFRASTRUCTURE ONLY.

The contract of include/tritd.h (tritd_admm_holdout_f64), restated.  Line
numbers are fast_robust_triple_tensor/triple_decomp_ADMM.m's.  With Omega the
`observed` mask (None = all true), H the `holdout` mask, patience >= 0 and
val_norm in {2, 1}:

* only H & Omega counts: a flag outside Omega is ignored, whatever D holds there;
* the fit is tests/masked_oracle.triple_decomp_ADMM_masked with Omega & ~H:
  with patience = 0 its A, B, C, O, E, errHist and k are that call's, bit for
  bit, and O and E are exactly 0 on H & Omega;
* with L_k = triple_product(A, B, C) after the updates of iteration k (:38),
    valHist(k)  = ||H o Omega o (D - L_k)|| / ||H o Omega o D||
    valHist1(k) = sum_{H & Omega} |D - L_k| / sum_{H & Omega} |D|,
  both truncated with errHist (:68);
* best_iter = the first minimum of the history val_norm picks (a strict <
  against the running best, k = 1 always taken); A_best, B_best, C_best are the
  factors after iteration best_iter;
* patience = p > 0: after the stop test of :63 for iteration k,
  k - best_iter >= p stops the loop at k like a reference stop;
* stop_reason: 0 ran to maxIter, 1 the test of :63, 2 patience.

The loop itself is masked_oracle's: it is run once with every iteration traced
(L_k, A, B, C), the scores and the bookkeeping are taken from the trace in
iteration order, and where patience stops the loop before the masked call would
have ended, the masked call is run again with maxIter = k (the same statements,
so the same bits) for the outputs of iteration k.
"""
from __future__ import annotations

import numpy as np

import masked_oracle as mo
import tritd_oracle as orc


def split_masks(D, observed, holdout):
    """(Omega & ~H, H & Omega) as column-major bool arrays of D's shape."""
    shape = orc.as3(D).shape
    W = np.ones(shape, dtype=bool) if observed is None else \
        (np.asarray(observed) != 0).reshape(shape, order="F")
    H = (np.asarray(holdout) != 0).reshape(shape, order="F")
    return np.asfortranarray(W & ~H), np.asfortranarray(H & W)


def scores(D, held, L):
    """(valHist, valHist1) of one L."""
    x = np.asarray(D)[held]
    d = x - np.asarray(L)[held]
    return (float(np.linalg.norm(d) / np.linalg.norm(x)),
            float(np.sum(np.abs(d)) / np.sum(np.abs(x))))


def triple_decomp_ADMM_holdout(D, observed, holdout, r, opts, A0, B0, C0, patience=0, val_norm=2):
    if holdout is None:
        raise ValueError("holdout is required")
    if patience < 0:
        raise ValueError("patience must be >= 0")
    if val_norm not in (1, 2):
        raise ValueError("val_norm must be 1 or 2")
    fit, held = split_masks(D, observed, holdout)
    if not held.any():
        raise ValueError("holdout has no observed entry: nothing to score")
    if not fit.any():
        raise ValueError("no observed entry is left to fit beside the holdout")
    D = orc.as3(D)
    if np.linalg.norm(D[held]) == 0.0:
        raise ValueError("the held-out entries of D are all zero")
    maxIter = int(opts["maxIter"])
    run = mo.triple_decomp_ADMM_masked(D, fit, r, opts, A0, B0, C0,
                                       trace_iters=range(1, maxIter + 1))
    k_ref, trace = run[6], run[7]

    valHist, valHist1 = np.zeros(k_ref), np.zeros(k_ref)
    best, best_iter, k, stop_reason = np.inf, 0, k_ref, 0
    for it in range(1, k_ref + 1):                    # in the loop's order
        valHist[it - 1], valHist1[it - 1] = scores(D, held, trace[it]["L"])
        v = valHist1[it - 1] if val_norm == 1 else valHist[it - 1]
        if it == 1 or v < best:
            best, best_iter = v, it
        if it == k_ref and k_ref < maxIter:
            stop_reason = 1                            # :63 broke the loop at k_ref
        elif it == k_ref and k_ref > 1 and \
                abs(run[4][-1] - run[4][-2]) < float(opts["tol"]) * run[4][-2]:
            stop_reason = 1                            # :63 fired in the last iteration
        elif patience > 0 and it - best_iter >= patience:
            k, stop_reason = it, 2
            break
    if k < k_ref:  # the outputs of iteration k: the same statements, ended at k
        run = mo.triple_decomp_ADMM_masked(D, fit, r, dict(opts, maxIter=k), A0, B0, C0)
        assert run[6] == k
    A, B, C, O, errHist, E = run[:6]
    tb = trace[best_iter]
    return dict(A=A, B=B, C=C, O=O, E=E, errHist=errHist, k=k, valHist=valHist[:k],
                valHist1=valHist1[:k], best_iter=best_iter, stop_reason=stop_reason,
                A_best=tb["A"], B_best=tb["B"], C_best=tb["C"], fit=fit, held_out=held)
