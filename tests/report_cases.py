"""Shared inputs of the session-report tests.

The fp64 cases of tests/foreground_cases.py (their shapes cover the edges of
the tile-major layout: 21 x 7 x 19 has pad rows, padded frames, a padded tile
group and n2 < 11, so SSIM is -Inf; 16 x 5 x 16 has no padding; 36 x 21 x 34
at r = 5 and r = 11 has three t-tiles and padded ranks 32 and 128; 70 x 33 x 5
has three runs of 64 tiles) and one Qi case at r = 2 (21 x 13 x 19: pad rows,
padded frames, frames larger than the SSIM window).  The original tensor X is
the case's D; 15 % of its entries are missing, drawn as the video driver draws
them (drivers.missing_mask: exactly round(0.15 numel) positions) and
zero-filled (video_triple_comparison.m:30-31).  ITERS = 10 iterations.

References are computed once per process and shared (lru_cache); callers must
not modify the arrays they get.  tests/test_report_cases.py admits every case
on the CPU oracle.
"""
import functools

import numpy as np

import foreground_cases as fc

ITERS = fc.ITERS
STEPS = (3, ITERS - 3)
MISSING_RATIO = 0.15
QI_CASE = "qi21_r2"
CASES = tuple(fc.F64_CASES) + (QI_CASE,)
_QI_SHAPE, _QI_R, _QI_SEED = (21, 13, 19), 2, 960


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(D, A0, B0, C0, opts, r, shape, model): D is the original tensor X"""
    if name != QI_CASE:
        c = fc.case(name)
        return dict(D=c["D"], A0=c["A0"], B0=c["B0"], C0=c["C0"], opts=c["opts"], r=c["r"],
                    shape=c["shape"], model="cp")
    from sweep_cases import active_lambda
    from tritd import synth
    n1, n2, n3 = _QI_SHAPE
    rng = np.random.default_rng(_QI_SEED)
    L = synth.qi_full(*synth.random_factors(n1, n2, n3, _QI_R, _QI_SEED + 1))
    L *= fc.BACKGROUND_STD / float(L.std())
    spikes = rng.random(_QI_SHAPE) < fc.SPIKE_SHARE
    mag = rng.uniform(0.3 * fc.THR, 4.0 * fc.THR, size=_QI_SHAPE) * rng.choice([-1.0, 1.0], size=_QI_SHAPE)
    D = np.asfortranarray(L + np.where(spikes, mag, 0.0))
    A0, B0, C0 = synth.random_factors(n1, n2, n3, _QI_R, _QI_SEED + 2)
    opts = dict(synth.TRAFFIC_OPTS, maxIter=ITERS, model="qi")
    opts["lambda"] = fc.LAMBDA_SCALE * active_lambda(D)
    return dict(D=D, A0=A0, B0=B0, C0=C0, opts=opts, r=_QI_R, shape=_QI_SHAPE, model="qi")


@functools.lru_cache(maxsize=None)
def missing(name):
    """the driver's mask of missing entries (True = missing), column-major"""
    from tritd import drivers
    seed = _QI_SEED + 3 if name == QI_CASE else fc.SEEDS[name] + 5
    return np.asfortranarray(drivers.missing_mask(case(name)["shape"], MISSING_RATIO,
                                                  np.random.default_rng(seed)))


@functools.lru_cache(maxsize=None)
def observed_data(name):
    """Y = X with the missing entries zeroed (:30-31)"""
    Y = np.array(case(name)["D"], dtype=np.float64, order="F", copy=True)
    Y[missing(name)] = 0.0
    return Y


@functools.lru_cache(maxsize=None)
def holdout(name):
    shape = case(name)["shape"]
    seed = _QI_SEED + 4 if name == QI_CASE else fc.SEEDS[name] + 6
    return np.asfortranarray(np.random.default_rng(seed).random(shape) < 0.10)


@functools.lru_cache(maxsize=None)
def oracle_run(name, masked):
    """(L, O) of the numpy oracle after ITERS iterations on Y: the reference
    solver (the zeros are data) or the masked one with observed = ~missing"""
    import tritd_oracle as orc
    c = case(name)
    if masked:
        from masked_oracle import triple_decomp_ADMM_masked
        out = triple_decomp_ADMM_masked(observed_data(name), ~missing(name), c["r"], c["opts"],
                                        c["A0"], c["B0"], c["C0"])
    else:
        out = orc.triple_decomp_ADMM(observed_data(name), c["r"], c["opts"], c["A0"], c["B0"], c["C0"])
    L = orc.triple_product(out[0], out[1], out[2], model=c["model"])
    return np.asfortranarray(L), np.asfortranarray(out[3])
