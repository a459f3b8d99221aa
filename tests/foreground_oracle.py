"""CPU oracle of the foreground detection — TEST INFRASTRUCTURE ONLY.

A numpy restatement of `eval`, video_triple_comparison.m:327-370, statement
for statement (the line numbers on the right).  `graythresh` of :335-336 is
computed there and never used; it is not restated.  The counts are int64 and
exact; the scores follow MATLAB's double arithmetic, 0/0 -> NaN included.
"""
import numpy as np


def pred_mask(F, thr=50.0):
    """:327-340: pred_mask(:,:,i) = abs(foreground(:,:,i)) > thr, frame by frame
    (dimensions past the second folded into frames).  A single F is widened to
    double for the comparison, which is exact."""
    F = np.asarray(F)
    n1 = F.shape[0]
    n2 = F.shape[1] if F.ndim > 1 else 1
    F3 = F.reshape((n1, n2, -1), order="F")
    pred = np.zeros(F3.shape, dtype=bool, order="F")                     # :327
    for i in range(F3.shape[2]):                                          # :329
        diff_img = np.abs(F3[:, :, i].astype(np.float64))                 # :333
        pred[:, :, i] = diff_img > thr                                    # :339 (NaN > thr is false)
    return pred.reshape(F.shape, order="F")


def eval_counts(F, G, thr=50.0):
    """:342-360 -> int64 (nf, 4): TP, FP, FN, TN of every frame."""
    F = np.asarray(F)
    G = np.asarray(G)
    assert F.shape == G.shape                                             # :320
    n1 = F.shape[0]
    n2 = F.shape[1] if F.ndim > 1 else 1
    pm = pred_mask(F, thr).reshape((n1, n2, -1), order="F")
    G3 = G.reshape((n1, n2, -1), order="F")
    gt_mask = G3 == 255                                                   # :342
    ns_mask = G3 == 170                                                   # :343
    nf = pm.shape[2]
    counts = np.zeros((nf, 4), dtype=np.int64)
    for i in range(nf):                                                   # :347
        p = pm[:, :, i].ravel(order="F")                                  # :348
        g = gt_mask[:, :, i].ravel(order="F")                             # :349
        m = ns_mask[:, :, i].ravel(order="F")                             # :350
        counts[i, 0] = np.sum(p & (g | m))                                # :351 TP
        counts[i, 1] = np.sum(p & ~g)                                     # :352 FP
        counts[i, 2] = np.sum(~p & g)                                     # :353 FN
        counts[i, 3] = np.sum(~p & (~g | m))                              # :354 TN
    return counts


def scores(counts, numel):
    """:356-365 from per-frame counts: dict(total, precision, recall, f1, pwc)."""
    total = np.asarray(counts, dtype=np.int64).reshape(-1, 4).sum(axis=0)  # :356-359
    TP, FP, FN = (np.float64(v) for v in total[:3])
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = TP / (TP + FP)                                        # :362
        recall = TP / (TP + FN)                                           # :363
        f1 = np.float64(2) * precision * recall / (precision + recall)    # :364
        pwc = np.float64(100) * (FP + FN) / np.float64(numel)             # :365
    return dict(total=total, precision=float(precision), recall=float(recall), f1=float(f1),
                pwc=float(pwc))


def report_lines(s):
    """The five lines of :366-370 (note the order TP, FP, TN, FN of :366)."""
    TP, FP, FN, TN = (int(v) for v in s["total"])
    return ["TP: %d FP: %d TN: %d FN: %d " % (TP, FP, TN, FN),
            "Precision: %.4f" % s["precision"],
            "Recall   : %.4f" % s["recall"],
            "F1 Score : %.4f" % s["f1"],
            "PWC      : %.4f%%" % s["pwc"]]
