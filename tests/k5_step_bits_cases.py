"""Shared inputs of the K5 step bit-for-bit tests (tests/test_gpu_k5_step_bits.py,
tests/test_k5_step_bits_cases.py, tests/golden/make_k5_step_bits.py).

Seven small fp64 ADMM problems whose fused update (K5, csrc/k_admm.hip) meets,
inside one wave's walk over the t-tiles of an ij-tile, compact-E slots and
overflowed (dense) E tiles side by side, at every padded rank RP <= 64:

    case            r  RP  shape      what it exercises
    r2_16x4x32      2  16  16x4x32    smallest padded rank
    r5_40x3x40      5  32  40x3x40    ragged rows, padded t, an inactive wave
    r7_24x5x48      7  64  24x5x48    49 rank columns padded to 64
    r8_64x4x64      8  64  64x4x64    the benchmark's rank
    r3_20x2x160     3  16  20x2x160   t-split walk (4 ij-tiles: two chunks of 5 t-tiles)
    r5_masked       5  32  40x3x40    masked form, 70 % of the entries observed
    r5_dense_e      5  32  40x3x40    forced dense-E form (TRITD_DENSE_E=1)

Each runs ITERS = 6 iterations, one-shot and stepped STEPS = 4 + 2, and every
output is compared at the iterations of COMPARED.  Data: a random low-rank
tensor plus outliers U(-10 sigma, 10 sigma) whose share alternates from one
t-tile to the next (P_HI of the entries where t // 16 is even, P_LO where it is
odd), so that a wave's walk passes through tiles that overflow their slot and
tiles that do not.  lambda = LAMBDA_STD * 1e-3 * std(D) (the threshold
lambda / mu starts at LAMBDA_STD std(D)) and rho = RHO, slower than the traffic
driver's 1.25: with that one the threshold falls threefold in six iterations and
E goes from all zeros to dense everywhere in between.  tests/
test_k5_step_bits_cases.py asserts on the CPU, with the numpy oracle and the
tile map of csrc/common.h, that between 10 % and 90 % of E's tiles hold more
than CE_CAP = 27 nonzeros at every compared iteration and that some walk holds
both kinds.
"""
import functools

import numpy as np

ITERS = 6
STEPS = (4, 2)
COMPARED = (4, 6)  # iterations after which the stepped session is read
CE_CAP = 27        # csrc/common.h: a tile with more nonzeros is stored densely
P_HI, P_LO = 0.35, 0.03
LAMBDA_STD = 1.5
RHO = 1.05
OBSERVED = 0.70
SHARE_BAND = (0.10, 0.90)

#        id              r  shape          masked dense_e seed
CASES = (("r2_16x4x32", 2, (16, 4, 32), False, False, 2),
         ("r5_40x3x40", 5, (40, 3, 40), False, False, 5),
         ("r7_24x5x48", 7, (24, 5, 48), False, False, 7),
         ("r8_64x4x64", 8, (64, 4, 64), False, False, 8),
         ("r3_20x2x160", 3, (20, 2, 160), False, False, 3),
         ("r5_masked", 5, (40, 3, 40), True, False, 5),
         ("r5_dense_e", 5, (40, 3, 40), False, True, 5))
IDS = tuple(c[0] for c in CASES)
_BY_ID = {c[0]: c for c in CASES}
# what a recording holds per case and compared iteration
KEYS = ("A", "B", "C", "O", "E", "errHist")


def padded_rank(r):
    return (r * r + 15) // 16 * 16


def tsplit(shape, r):
    """k5_tsplit of csrc/k_admm.hip for a problem this small (fewer than 256
    workgroups): chunks of at least 4 t-tiles."""
    n1, n2, n3 = shape
    wg = -(-((n1 + 15) // 16 * n2) // 4)
    ntt = (n3 + 15) // 16
    return max(1, min(-(-256 // wg), max(ntt // 4, 1)))


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """dict(D, A0, B0, C0, opts, r, observed (or None), dense_e, id).  Callers
    must not modify the arrays."""
    from tritd import synth
    _, r, shape, masked, dense_e, seed = _BY_ID[cid]
    n3 = shape[2]
    L = synth.cp_full(*synth.hat_factors(*synth.random_factors(*shape, r, seed)))
    sigma = float(L.std())
    rng = np.random.default_rng([seed, 1])
    p = np.where((np.arange(n3) // 16) % 2 == 0, P_HI, P_LO)[None, None, :]
    support = rng.random(shape) < p
    vals = rng.uniform(-10.0 * sigma, 10.0 * sigma, size=shape)
    A0, B0, C0 = synth.random_factors(*shape, r, seed + 100)
    d = dict(D=np.asfortranarray(L + np.where(support, vals, 0.0)), A0=A0, B0=B0, C0=C0)
    opts = dict(synth.TRAFFIC_OPTS, maxIter=ITERS, tol=0.0, rho=RHO)
    opts["lambda"] = LAMBDA_STD * 1e-3 * float(np.std(d["D"]))
    obs = None
    if masked:
        obs = np.asfortranarray(np.random.default_rng([seed, 11]).random(shape) < OBSERVED)
    return dict(D=d["D"], A0=d["A0"], B0=d["B0"], C0=d["C0"], opts=opts, r=r, observed=obs,
                dense_e=dense_e, id=cid)


@functools.lru_cache(maxsize=None)
def oracle_E(cid, iters):
    """E of the numpy oracle after `iters` iterations."""
    c = inputs(cid)
    o = dict(c["opts"], maxIter=iters)
    if c["observed"] is not None:
        import masked_oracle as mo
        return mo.triple_decomp_ADMM_masked(c["D"], c["observed"], c["r"], o, c["A0"], c["B0"], c["C0"])[5]
    import tritd_oracle as orc
    return orc.triple_decomp_ADMM(c["D"], c["r"], o, c["A0"], c["B0"], c["C0"])[5]


def tile_counts(E):
    """Nonzeros of every E tile in the tile map of csrc/common.h: tile (g, tt)
    is 16 consecutive (zero-padded) rows i of one fibre j, g = (j n1p + i)/16,
    by the 16 (zero-padded) t of t-tile tt.  Shape (ij-tiles, t-tiles)."""
    E = np.asarray(E)
    n1, n2, n3 = E.shape
    n1p, n3p = (n1 + 15) // 16 * 16, (n3 + 15) // 16 * 16
    P = np.zeros((n1p, n2, n3p), dtype=bool)
    P[:n1, :, :n3] = E != 0
    # (ib, 16, j, tt, 16) -> counts[j, ib, tt] -> g = j * (n1p/16) + ib
    cnt = P.reshape(n1p // 16, 16, n2, n3p // 16, 16).sum(axis=(1, 4))
    return np.transpose(cnt, (1, 0, 2)).reshape(n2 * (n1p // 16), n3p // 16)


def dense_share(E):
    """Share of E's tiles that overflow their compact slot (> CE_CAP nonzeros)."""
    return float(np.mean(tile_counts(E) > CE_CAP))


def mixed_walks(E, chunks=1):
    """Number of walks (one wave: an ij-tile's t-tiles of one t-split chunk,
    t0 = c ntt / chunks as in k5_fused) that hold both tile kinds."""
    over = tile_counts(E) > CE_CAP
    ntt = over.shape[1]
    n = 0
    for c in range(chunks):
        w = over[:, c * ntt // chunks:(c + 1) * ntt // chunks]
        n += int(np.sum(w.any(axis=1) & ~w.all(axis=1)))
    return n
