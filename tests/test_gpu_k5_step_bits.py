"""K5's step, bit for bit: the seven cases of tests/k5_step_bits_cases.py (every
padded rank up to 64, ragged rows, padded t, an inactive wave, the t-split walk,
the masked form and the forced dense-E form; compact slots and overflowed tiles
inside one wave's walk, asserted on the CPU by tests/test_k5_step_bits_cases.py)
run 6 iterations through the one-shot call and through a Session stepped 4 + 2,
and A, B, C, O, E and errHist must equal, bit for bit, the recordings of
tests/golden/k5_step_bits.npz (tests/golden/make_k5_step_bits.py: made once on
the GPU from the build before the step's instruction stream was rearranged —
the encode as one basic block, the L chain ahead of the decodes, the
nontemporal slot loads).  The dense-tile counter must match
too: the same tiles overflowed.

The recordings hold O and E in full after the last iteration and as SHA-256
digests of their bytes after the intermediate one (the file stays within the
size limit of a committed file); everything else in full at both.
"""
import contextlib
import hashlib
import os

import numpy as np
import pytest

import k5_step_bits_cases as kc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DIGESTED = ("O", "E")  # at the intermediate iterations


def bits(a):
    """The array's bytes in column-major order."""
    return np.asarray(a).tobytes(order="F")


def digest(a):
    return np.frombuffer(hashlib.sha256(bits(a)).digest(), dtype=np.uint8)


def recorded(key, k, a):
    """What the recording holds for output `key` after iteration k."""
    return digest(a) if key in DIGESTED and k != kc.COMPARED[-1] else np.asarray(a)


@contextlib.contextmanager
def case_env(cid):
    """TRITD_DENSE_E=1 around the dense-E case (read at session creation)."""
    old = os.environ.get("TRITD_DENSE_E")
    if kc.inputs(cid)["dense_e"]:
        os.environ["TRITD_DENSE_E"] = "1"
    else:
        os.environ.pop("TRITD_DENSE_E", None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("TRITD_DENSE_E", None)
        else:
            os.environ["TRITD_DENSE_E"] = old


def run_one_shot(tritd, cid):
    c = kc.inputs(cid)
    A, B, C, O, eh, E, k = tritd.triple_decomp_ADMM(c["D"], c["r"], c["opts"], c["A0"], c["B0"], c["C0"],
                                                    device=0, return_E=True, return_iters=True,
                                                    observed=c["observed"])
    assert k == kc.ITERS
    return dict(A=A, B=B, C=C, O=O, E=E, errHist=np.asarray(eh))


def run_stepped(tritd, cid):
    """{iteration: outputs + dense (tiles stored densely so far, tiles per launch)}."""
    c = kc.inputs(cid)
    n1, n2, n3 = c["D"].shape
    s = tritd.Session(c["r"], c["opts"], c["A0"], c["B0"], c["C0"], n1=n1, n2=n2, n3=n3, D=c["D"],
                      device=0, probe=False, observed=c["observed"])
    out, k = {}, 0
    try:
        for step in kc.STEPS:
            s.run(step)
            k += step
            x = s.get()
            assert x["k"] == k
            out[k] = dict({key: x[key] for key in kc.KEYS}, dense=s.counters())
    finally:
        s.close()
    return out


@pytest.fixture(scope="module")
def tritd():
    import tritd as t
    assert t.device_count() > 0, "no GPU visible: the HIP path must run, there is no CPU fallback"
    return t


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "k5_step_bits.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def compare(golden, cid, k, got, label):
    bad = []
    for key in kc.KEYS:
        want = golden["%s/%d/%s" % (cid, k, key)]
        have = recorded(key, k, got[key])
        same = have.shape == want.shape and have.dtype == want.dtype and bits(have) == bits(want)
        if not same:
            n = int(np.sum(have != want)) if have.shape == want.shape else -1
            bad.append("%s (%d differ)" % (key, n))
    print("  k5 bits %s %s k=%d: %s" % (cid, label, k, "identical" if not bad else ", ".join(bad)), flush=True)
    assert not bad, "%s %s after iteration %d differs from the recording: %s" % (cid, label, k, bad)


@pytest.mark.parametrize("cid", kc.IDS)
def test_one_shot_bits(tritd, golden, cid):
    with case_env(cid):
        got = run_one_shot(tritd, cid)
    compare(golden, cid, kc.COMPARED[-1], got, "one-shot")


@pytest.mark.parametrize("cid", kc.IDS)
def test_stepped_bits(tritd, golden, cid):
    with case_env(cid):
        got = run_stepped(tritd, cid)
    assert tuple(got) == kc.COMPARED
    for k in kc.COMPARED:
        compare(golden, cid, k, got[k], "stepped")
        want = tuple(int(v) for v in golden["%s/%d/dense" % (cid, k)])
        assert tuple(got[k]["dense"]) == want, (cid, k, got[k]["dense"], want)
    c = kc.inputs(cid)
    dense, per = got[kc.ITERS]["dense"]
    if not c["dense_e"]:
        # slot overflow really occurred, and not everywhere
        assert 0 < dense < kc.ITERS * per, (dense, per)
