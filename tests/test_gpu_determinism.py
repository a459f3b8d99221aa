"""Run-to-run determinism of the HIP path: every reduction has a fixed order,
so the same solve twice must agree BITWISE.  A store that loses data now and
then (round 4: the dense-E K5 form wrote a wrong first word in lanes 12-15 of a
few Y_L stores per launch, k_admm.hip `keep`) shows up here as a difference
between repeats even when it stays inside the parity tolerances.

Shapes: config 3's frame size with 64 frames in the forced dense-E form and
in the compact form (1 200 K5 workgroups, several rounds of the GPU), the
traffic shape at 256^3 r = 8, and the fp32 r = 16 path.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0
    return t


def _solve(tritd, D, r, opts, d, env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return tritd.triple_decomp_ADMM(D, r, opts, d["A0"], d["B0"], d["C0"], return_E=True,
                                        return_iters=True)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(a, b):
    for x, y in zip(a[:6], b[:6]):
        assert np.array_equal(np.asarray(x), np.asarray(y)), "repeat differs"
    assert a[6] == b[6]


@pytest.mark.parametrize("dense_e", ["1", "0"])
def test_config3_frames_repeat_bitwise(tritd, dense_e):
    from tritd import synth
    d = synth.video_like(240, 320, 64, 5)
    opts = dict(synth.VIDEO_OPTS, maxIter=4)
    env = {"TRITD_DENSE_E": dense_e}
    first = _solve(tritd, d["D"], 5, opts, d, env)
    for _ in range(3):
        _same(_solve(tritd, d["D"], 5, opts, d, env), first)


def _active(opts, D, e_active):
    """lambda = 2e-3 std(D) (threshold 2 std(D) instead of 1800): E is nonzero
    within the few iterations of these cases.  With lambda = 1.8 it stays
    identically zero, and the E stores — where a store would be lost — write
    nothing that a repeat could differ in."""
    if e_active:
        opts = dict(opts)
        opts["lambda"] = 2e-3 * float(np.std(D))
    return opts


def _traffic_256(tritd, e_active):
    from tritd import synth
    d = synth.low_rank_plus_outliers(256, 256, 256, 8, seed=3)
    opts = _active(dict(synth.TRAFFIC_OPTS, maxIter=4), d["D"], e_active)
    first = _solve(tritd, d["D"], 8, opts, d, {})
    _same(_solve(tritd, d["D"], 8, opts, d, {}), first)
    if e_active:
        assert np.any(first[5])


def test_traffic_256_repeat_bitwise(tritd):
    _traffic_256(tritd, False)


def test_traffic_256_repeat_bitwise_e_active(tritd):
    _traffic_256(tritd, True)


def _f32_r16(tritd, e_active):
    from tritd import synth
    d = synth.low_rank_plus_outliers(256, 256, 64, 16, seed=4)
    opts = _active(dict(synth.TRAFFIC_OPTS, maxIter=3), d["D"], e_active)
    D = d["D"].astype(np.float32)
    first = _solve(tritd, D, 16, opts, d, {})
    _same(_solve(tritd, D, 16, opts, d, {}), first)
    if e_active:
        assert np.any(first[5])


def test_f32_r16_repeat_bitwise(tritd):
    _f32_r16(tritd, False)


def test_f32_r16_repeat_bitwise_e_active(tritd):
    _f32_r16(tritd, True)


# 96: 6 i-tiles, the two-tile form (k_tp2); 90: the same form with 6 padded
# rows in its last i-tile (row mask, paired stores of a partial tile; ADVICE
# r5); 80: 5 i-tiles, the one-tile form
@pytest.mark.parametrize("n1", [96, 90, 80])
def test_triple_product_repeat_bitwise(tritd, n1):
    """`triple_product` (k_tp2 pairs accumulator rows across lanes before its
    stores) twice on the same factors: bitwise equal, and within rounding of
    the oracle's product (triple_product.m:6)."""
    rng = np.random.default_rng(7)
    r = 8
    A = rng.standard_normal((n1, r, r))
    B = rng.standard_normal((r, 72, r))
    C = rng.standard_normal((r, r, 40))
    L1 = tritd.triple_product(A, B, C)
    L2 = tritd.triple_product(A, B, C)
    assert np.array_equal(L1, L2), "repeat differs"
    import tritd_oracle as orc
    ref = orc.triple_product(A, B, C)
    assert np.max(np.abs(L1 - ref)) <= 1e-12 * np.max(np.abs(ref))
