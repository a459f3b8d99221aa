"""The cases of tests/k5_step_bits_cases.py really put K5's two E tile kinds
side by side (checked here on the CPU, with the numpy oracle and the tile map
of csrc/common.h, so that a case that loses the dense path fails without a
GPU): after every compared iteration between 10 % and 90 % of E's tiles hold
more than CE_CAP = 27 nonzeros, and at least one wave's walk (an ij-tile's
t-tiles of one t-split chunk) holds both kinds.  The forced dense-E case takes
the data of the case it shares its shape with; the kernel it runs stores every
tile densely, whatever the counts."""
import re

import numpy as np
import pytest

import k5_step_bits_cases as kc
from conftest import PKG

MIXED = [c for c in kc.IDS if not kc.inputs(c)["dense_e"]]


def test_the_table_of_the_cases():
    got = [(c[1], kc.padded_rank(c[1]), c[2]) for c in kc.CASES]
    assert got == [(2, 16, (16, 4, 32)), (5, 32, (40, 3, 40)), (7, 64, (24, 5, 48)), (8, 64, (64, 4, 64)),
                   (3, 16, (20, 2, 160)), (5, 32, (40, 3, 40)), (5, 32, (40, 3, 40))]
    assert [c[3:5] for c in kc.CASES] == [(False, False)] * 5 + [(True, False), (False, True)]
    assert kc.ITERS == 6 and sum(kc.STEPS) == 6 and kc.COMPARED[-1] == 6
    # only the t-split case splits its walk; its chunks hold more than one t-tile
    assert [kc.tsplit(c[2], c[1]) for c in kc.CASES] == [1, 1, 1, 1, 2, 1, 1]
    # ragged rows with an inactive wave: 9 ij-tiles, the last workgroup has one
    n1, n2, _ = kc.CASES[1][2]
    assert n1 % 16 and ((n1 + 15) // 16 * n2) % 4 == 1


def test_ce_cap_is_the_kernels():
    text = open(PKG + "/csrc/common.h").read()
    assert int(re.search(r"constexpr int CE_CAP = (\d+);", text).group(1)) == kc.CE_CAP


def test_the_mask_observes_seventy_percent():
    obs = kc.inputs("r5_masked")["observed"]
    assert abs(obs.mean() - kc.OBSERVED) < 0.02


@pytest.mark.parametrize("cid", MIXED)
def test_tile_kinds_meet_at_every_compared_iteration(cid):
    _, r, shape, *_ = kc._BY_ID[cid]
    for k in kc.COMPARED:
        E = kc.oracle_E(cid, k)
        share, mixed = kc.dense_share(E), kc.mixed_walks(E, kc.tsplit(shape, r))
        print("  %s k=%d: %.0f %% of the tiles over %d nonzeros, %d mixed walks, nnz(E) %.3f"
              % (cid, k, 100 * share, kc.CE_CAP, mixed, np.count_nonzero(E) / E.size))
        assert kc.SHARE_BAND[0] <= share <= kc.SHARE_BAND[1], (cid, k, share)
        assert mixed >= 1, (cid, k)
        if kc.inputs(cid)["observed"] is not None:
            assert not np.any(E[~kc.inputs(cid)["observed"]])


def test_tile_counts_follow_the_tile_map():
    """tile (g, tt) of tile_counts against a direct count over tm_offset's map."""
    rng = np.random.default_rng(0)
    E = (rng.random((20, 3, 40)) < 0.2).astype(float)
    cnt = kc.tile_counts(E)
    n1p = 32
    assert cnt.shape == (3 * n1p // 16, 3)
    for i, j, t in [(0, 0, 0), (17, 1, 33), (19, 2, 39), (15, 2, 16)]:
        g, tt = (j * n1p + i) // 16, t // 16
        i0 = i // 16 * 16
        assert cnt[g, tt] == np.count_nonzero(E[i0:i0 + 16, j, tt * 16:tt * 16 + 16])
    assert cnt.sum() == np.count_nonzero(E)
