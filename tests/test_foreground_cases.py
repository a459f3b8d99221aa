"""CPU admission of tests/foreground_cases.py and of tests/foreground_oracle.py:
no GPU test of the foreground detection can pass vacuously.

Per case, on the oracle's O alone (after 3 and after ITERS iterations, the two
points at which tests/test_gpu_foreground.py looks):
* the predicted-positive share lies in [1 %, 50 %];
* the totals TP, FP, FN, TN are all > 0;
* some pixel has (G == 170) & p and some pixel (G == 170) & ~p;
* at least one frame has no 255;
* no |O| lies within GAP * thr of thr.  The issue of record asks for 1e-9 thr;
  GAP = 1e-6 asks more: the GPU's fp64 O agrees with the oracle's to ~1e-13
  relative, so a mask taken from either is the same mask.  The same holds for
  the masked case, where also O = 0 at every unobserved entry.
Plus the oracle's scores on a hand-worked two-frame example with the 0/0 cases,
and the overlap identity per frame.  By :351-354 a pixel with m (where g is
false, the two labels being different values) is counted twice when it is
predicted, as TP and as FP, and once when it is not, as TN alone (~g | m is
~g there): TP + FP + FN + TN = numel + #(m & p), not numel + #m.
"""
import math

import numpy as np
import pytest

import foreground_cases as fc
import foreground_oracle as fo

GAP = 1e-6
MASKED_CASE = "sweep36_r5"


@pytest.mark.parametrize("iters", [3, fc.ITERS])
@pytest.mark.parametrize("name", list(fc.CASES))
def test_case_is_admitted(name, iters):
    c = fc.case(name)
    O, G = fc.oracle_O(name, iters), c["G"]
    assert O.shape == G.shape == c["shape"] and G.dtype == np.uint8
    assert set(np.unique(G)) <= set(fc.LABELS)
    p = fo.pred_mask(O, fc.THR)
    share = p.mean()
    assert 0.01 <= share <= 0.50, share
    total = fo.scores(fo.eval_counts(O, G, fc.THR), O.size)["total"]
    assert (total > 0).all(), total
    m = G == 170
    assert (m & p).any() and (m & ~p).any()
    assert not (G[:, :, c["quiet_frame"]] == 255).any()
    assert any((G[:, :, t] == 255).any() for t in range(G.shape[2]))
    gap = np.min(np.abs(np.abs(O) - fc.THR)) / fc.THR
    assert gap >= GAP, gap


def test_spikes_span_the_threshold():
    """magnitudes from 0.3 thr to 4 thr, and labels that miss in both directions"""
    for name in fc.CASES:
        c = fc.case(name)
        D = c["D"].astype(np.float64)
        big = np.abs(D[c["spikes"]])
        assert big.max() > 3.0 * fc.THR and big.min() < fc.THR
        G = c["G"]
        assert ((G == 255) & ~c["spikes"]).any(), "no 255 away from the spikes"
        assert ((G == 0) & c["spikes"]).any(), "no spike on a 0 label"


@pytest.mark.parametrize("iters", [3, fc.ITERS])
def test_masked_case_is_admitted(iters):
    O = fc.oracle_O_masked(MASKED_CASE, iters)
    obs = fc.observed_mask(MASKED_CASE)
    assert 0.10 <= (~obs).mean() <= 0.25 and not obs[:16, 1, :16].any()
    assert (O[~obs] == 0).all()
    p = fo.pred_mask(O, fc.THR)
    assert 0.01 <= p.mean() <= 0.50
    assert np.min(np.abs(np.abs(O) - fc.THR)) / fc.THR >= GAP


def test_scores_hand_worked():
    # frame 0: TP 3, FP 1, FN 2, TN 10; frame 1: TP 1, FP 0, FN 0, TN 3
    s = fo.scores([[3, 1, 2, 10], [1, 0, 0, 3]], 20)
    assert list(s["total"]) == [4, 1, 2, 13]
    assert s["precision"] == 4 / 5 and s["recall"] == 4 / 6
    assert s["f1"] == 2 * (4 / 5) * (4 / 6) / (4 / 5 + 4 / 6)
    assert s["pwc"] == 100 * 3 / 20
    # nothing predicted and nothing to find: 0/0 everywhere but PWC
    z = fo.scores(np.zeros((2, 4), dtype=np.int64), 8)
    assert math.isnan(z["precision"]) and math.isnan(z["recall"]) and math.isnan(z["f1"])
    assert z["pwc"] == 0.0
    # predictions, none right: precision 0, recall 0/0, F1 NaN
    w = fo.scores([[0, 5, 0, 3]], 8)
    assert w["precision"] == 0.0 and math.isnan(w["recall"]) and math.isnan(w["f1"])
    # no pixels at all: PWC 0/0
    assert math.isnan(fo.scores(np.zeros((0, 4), dtype=np.int64), 0)["pwc"])
    assert fo.report_lines(s) == ["TP: 4 FP: 1 TN: 13 FN: 2 ", "Precision: 0.8000",
                                  "Recall   : 0.6667", "F1 Score : 0.7273", "PWC      : 15.0000%"]


def test_counts_hand_worked():
    F = np.array([[60.0, -60.0, 10.0, 50.0], [np.nan, 70.0, -80.0, 0.0]]).T.reshape((4, 1, 2), order="F")
    G = np.array([[255, 170, 255, 0], [255, 0, 170, 170]], dtype=np.uint8).T.reshape((4, 1, 2), order="F")
    # frame 0: p = 1 1 0 0; g = 1 0 1 0; m = 0 1 0 0
    # frame 1: p = 0 1 1 0; g = 1 0 0 0; m = 0 0 1 1
    assert fo.eval_counts(F, G, 50.0).tolist() == [[2, 1, 1, 1], [1, 2, 1, 1]]


@pytest.mark.parametrize("name", list(fc.CASES))
def test_overlap_identity(name):
    """every predicted pixel with m is counted twice, by the definitions of :351-354"""
    G, O = fc.case(name)["G"], fc.oracle_O(name)
    counts = fo.eval_counts(O, G, fc.THR)
    p = fo.pred_mask(O, fc.THR)
    n1, n2, n3 = G.shape
    twice = 0
    for t in range(n3):
        mp = np.count_nonzero((G[:, :, t] == 170) & p[:, :, t])
        assert counts[t].sum() == n1 * n2 + mp
        twice += mp
    assert twice > 0


def test_special_values_cover_the_comparison():
    F, G = fc.special_values(fc.THR)
    assert F.shape == (20, 3, 5)
    p = fo.pred_mask(F, fc.THR)
    assert not p[np.isnan(F)].any() and p[np.isinf(F)].all()
    assert not p[np.abs(F) == fc.THR].any() and (np.abs(F) == fc.THR).sum() >= 2
    assert p[F == np.nextafter(fc.THR, np.inf)].all()
    assert not p[F == np.nextafter(fc.THR, -np.inf)].any()
    # thr = 0: only exact zeros (of either sign) and NaN are negative
    p0 = fo.pred_mask(F, 0.0)
    assert (p0 == ((F != 0) & ~np.isnan(F))).all() and p0[np.abs(F) == 5e-324].all()
