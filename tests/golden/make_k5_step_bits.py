"""Records tests/golden/k5_step_bits.npz: every output of the seven cases of
tests/k5_step_bits_cases.py after the iterations of COMPARED, from the library
that is built in the tree, on the GPU.  Outputs only (the inputs are
regenerated from their seeds).  A, B, C, O, E as float64 bit patterns, errHist
as it is; the dense-tile counter of the stepped session beside them.

Run it on the commit whose bits are to be pinned (the recordings in the
repository come from the parent of the commit that added this file), never to
make a failing comparison pass.

    python tests/golden/make_k5_step_bits.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"),
          os.path.join(ROOT, "triple-tensor-decomposition-with-admm_amd")):
    sys.path.insert(0, p)

import k5_step_bits_cases as kc  # noqa: E402
import test_gpu_k5_step_bits as tg  # noqa: E402


def main():
    import tritd
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "k5_step_bits.npz")
    rec = {}
    for cid in kc.IDS:
        with tg.case_env(cid):
            stepped = tg.run_stepped(tritd, cid)
            one = tg.run_one_shot(tritd, cid)
        last = kc.COMPARED[-1]
        for key in kc.KEYS:
            assert tg.bits(one[key]) == tg.bits(stepped[last][key]), (cid, key, "one-shot != stepped")
        for k in kc.COMPARED:
            for key in kc.KEYS:
                rec["%s/%d/%s" % (cid, k, key)] = tg.recorded(key, k, stepped[k][key])
            rec["%s/%d/dense" % (cid, k)] = np.array(stepped[k]["dense"], dtype=np.int64)
        E = stepped[last]["E"]
        print("%s: nnz(E) %.3f, dense tiles %s of %d per launch, errHist[-1] %.6e"
              % (cid, np.count_nonzero(E) / E.size, stepped[last]["dense"][0], stepped[last]["dense"][1],
                 stepped[last]["errHist"][-1]), flush=True)
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
