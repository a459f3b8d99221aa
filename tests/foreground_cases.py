"""Shared inputs of the foreground-detection tests.

A case is a rank-r background plus sparse spikes whose magnitudes are spread
from 0.3 thr to 4 thr, solved for ITERS iterations with an active lambda
(LAMBDA_SCALE x sweep_cases.active_lambda: the soft threshold starts at
0.2 std(D), so E takes the spikes out of the fit from the first iterations
and O keeps them; with the 2 std(D) of the sweep a rank-256 model of these
small tensors absorbs every spike and abs(O) never reaches thr), and a
ground truth G of CDnet labels {0, 50, 85, 170, 255}: 255 and 170 sit on and
around the spikes, some 255 fall away from them (false negatives), some spikes
fall on 0 (false positives), and one frame has no 255 at all.  The foreground
of a case is the O of the fixed-order oracle (oracle/tritd_oracle.py; the
masked form: tests/masked_oracle.py).  tests/test_foreground_cases.py admits
every case on the CPU: none can let a GPU test pass vacuously.

Shapes, for the edges of the tile-major layout (16 rows x 16 frames per tile,
groups of four ij-tiles):
    21 x 7 x 19   n1p = 32 with pad rows, 14 ij-tiles (the last group is
                  padded), two t-tiles with 13 padded frames
    16 x 5 x 16   no padding at all, 5 ij-tiles
    36 x 21 x 34  the size of sweep_cases, three t-tiles: several workgroups
    70 x 33 x 5   165 ij-tiles: three runs of 64 tiles, the last one short
Ranks: r = 5 (fp64, padded rank <= 64), r = 11 (fp64, padded rank 128),
r = 16 (the fp32 path's padded rank 256); fp32 at r = 5 too, on the padded
shape (at r = 16 a tensor of 21 x 7 x 19 is fitted exactly and O stays under thr).

References are computed once per process and shared (lru_cache); callers must
not modify the arrays they get.
"""
import functools

import numpy as np

THR = 50.0  # video_triple_comparison.m:339
ITERS = 10
LABELS = (0, 50, 85, 170, 255)

# name -> (shape, r, dtype of D)
CASES = {
    "pad21_r5": ((21, 7, 19), 5, np.float64),
    "full16_r5": ((16, 5, 16), 5, np.float64),
    "sweep36_r5": ((36, 21, 34), 5, np.float64),
    "runs70_r5": ((70, 33, 5), 5, np.float64),
    "sweep36_r11": ((36, 21, 34), 11, np.float64),
    "pad21_r5_f32": ((21, 7, 19), 5, np.float32),
    "sweep36_r16_f32": ((36, 21, 34), 16, np.float32),
}
F64_CASES = tuple(n for n, c in CASES.items() if c[2] == np.float64)
F32_CASES = tuple(n for n, c in CASES.items() if c[2] == np.float32)
SEEDS = {n: 900 + q for q, n in enumerate(CASES)}
SPIKE_SHARE = 0.08
BACKGROUND_STD = 12.0  # of the low-rank part, well under thr
LAMBDA_SCALE = 0.1


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(D, A0, B0, C0, opts, r, G, spikes, shape, f32): D column-major of the
    case's dtype, G uint8 of D's shape, spikes the logical support."""
    from sweep_cases import active_lambda
    from tritd import synth
    shape, r, dtype = CASES[name]
    n1, n2, n3 = shape
    rng = np.random.default_rng(SEEDS[name])
    As, Bs, Cs = synth.random_factors(n1, n2, n3, r, SEEDS[name] + 1)
    L = synth.cp_full(*synth.hat_factors(As, Bs, Cs))
    L *= BACKGROUND_STD / float(L.std())
    spikes = rng.random(shape) < SPIKE_SHARE
    mag = rng.uniform(0.3 * THR, 4.0 * THR, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    D = np.asfortranarray((L + np.where(spikes, mag, 0.0)).astype(dtype))
    A0, B0, C0 = synth.random_factors(n1, n2, n3, r, SEEDS[name] + 2)
    opts = dict(synth.TRAFFIC_OPTS, maxIter=ITERS)
    opts["lambda"] = LAMBDA_SCALE * active_lambda(D)

    # labels: a background of 0 / 50 / 85, 255 (70 %) / 170 (10 %) / 0 (20 %) on
    # the spikes, 170 on a third of their row neighbours, 255 on 1 % of the rest
    G = rng.choice(np.array([0, 50, 85], dtype=np.uint8), size=shape, p=[0.8, 0.1, 0.1])
    near = np.zeros(shape, dtype=bool)
    near[1:] |= spikes[:-1]
    near[:-1] |= spikes[1:]
    near &= ~spikes
    G[near & (rng.random(shape) < 1.0 / 3.0)] = 170
    G[~spikes & ~near & (rng.random(shape) < 0.01)] = 255
    u = rng.random(shape)
    G[spikes & (u < 0.7)] = 255
    G[spikes & (u >= 0.7) & (u < 0.8)] = 170
    G[spikes & (u >= 0.8)] = 0
    quiet = n3 // 2  # one frame without a 255
    G[:, :, quiet][G[:, :, quiet] == 255] = 0
    return dict(D=D, A0=A0, B0=B0, C0=C0, opts=opts, r=r, G=np.asfortranarray(G), spikes=spikes,
                shape=shape, f32=dtype == np.float32, quiet_frame=quiet)


@functools.lru_cache(maxsize=None)
def oracle_O(name, iters=ITERS):
    """O of the fixed-order numpy oracle after `iters` iterations (fp64; for a
    float32 case the oracle runs in double on the float32 data)."""
    import tritd_oracle as orc
    c = case(name)
    out = orc.triple_decomp_ADMM(np.asfortranarray(c["D"], dtype=np.float64), c["r"],
                                 dict(c["opts"], maxIter=iters), c["A0"], c["B0"], c["C0"])
    return np.asfortranarray(out[3])


@functools.lru_cache(maxsize=None)
def observed_mask(name):
    """15 % of the entries missing, and one whole 16 x 16 (i, t) tile of fibre
    j = 1 (rows 0..15, frames 0..15)."""
    shape = CASES[name][0]
    rng = np.random.default_rng(SEEDS[name] + 3)
    obs = rng.random(shape) >= 0.15
    obs[:16, 1, :16] = False
    return np.asfortranarray(obs)


@functools.lru_cache(maxsize=None)
def holdout_mask(name):
    shape = CASES[name][0]
    rng = np.random.default_rng(SEEDS[name] + 4)
    return np.asfortranarray(rng.random(shape) < 0.10)


@functools.lru_cache(maxsize=None)
def oracle_O_masked(name, iters=ITERS):
    from masked_oracle import triple_decomp_ADMM_masked
    c = case(name)
    out = triple_decomp_ADMM_masked(c["D"], observed_mask(name), c["r"],
                                    dict(c["opts"], maxIter=iters), c["A0"], c["B0"], c["C0"])
    return np.asfortranarray(out[3])


def special_values(thr):
    """20 x 3 x 5 of the values a comparison can get wrong, around `thr`, and
    labels that cycle through LABELS: -> (F float64, G uint8)."""
    vals = [np.nan, np.inf, -np.inf, -0.0, 0.0, thr, -thr, np.nextafter(thr, np.inf),
            np.nextafter(thr, -np.inf), -np.nextafter(thr, np.inf), -np.nextafter(thr, -np.inf),
            2.0 * thr + 1.0, -3.0 * thr - 1.0, 5e-324, -5e-324, 1e308, -1e308, 0.5 * thr,
            np.float64(np.float32(thr)), -np.float64(np.nextafter(np.float32(thr), np.float32(np.inf)))]
    F = np.resize(np.array(vals, dtype=np.float64), 20 * 3 * 5).reshape((20, 3, 5), order="F")
    G = np.resize(np.array(LABELS * 3 + (255, 170), dtype=np.uint8), F.size).reshape(F.shape, order="F")
    return np.asfortranarray(F), np.asfortranarray(G)
