"""The compiled pair loop of the benchmark's K5 keeps its scheduling regions:
tools/k5_regions.py on the built libtritd.so finds no more conditional branches
in the loop than profiles/k5_step_regions/regions_branch.txt records (its last
line, `cbranch N`), and the loop still holds the two t-tiles' 64 MFMAs.  A
source change that makes the compiler cut the compact-E encode into scalar
control flow again (a branch per mask word, a lane-masked
stretch for the count word) fails here, without a GPU."""
import os
import re
import sys

import pytest

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import k5_regions as kr  # noqa: E402
import scan_store_war as sw  # noqa: E402

LIB = os.path.join(PKG, "tritd", "libtritd.so")
RECORD = os.path.join(ROOT, "profiles", "k5_step_regions", "regions_branch.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(f"{sw.LLVM}/llvm-objdump"),
                                reason="llvm-objdump not installed")


def recorded(name):
    return int(re.search(r"^%s (\d+)$" % name, open(RECORD).read(), re.M).group(1))


@pytest.fixture(scope="module")
def rep():
    assert os.path.exists(LIB), "build libtritd.so first (__graft_entry__.build())"
    return kr.report(LIB)


def test_the_pair_loop_is_found(rep):
    assert "k5_fusedILi64ELb0ELb0ELb0EE" in rep["kernel"]
    assert rep["totals"]["mfma"] == 64  # (16 for L + 16 for W) x two t-tiles


def test_no_more_conditional_branches_than_recorded(rep):
    print("  pair loop: %d conditional branches (recorded %d), %d saveexec (recorded %d)"
          % (rep["cbranch"], recorded("cbranch"), rep["saveexec"], recorded("saveexec")))
    assert rep["cbranch"] <= recorded("cbranch")
    assert rep["saveexec"] <= recorded("saveexec")


def test_regions_of_a_synthetic_loop():
    """The region cutter on a hand-made listing: a loop of three regions."""
    ins = [(0, "v_mov_b32", ["v0", "v1"]),
           (4, "v_mfma_f64_16x16x4_f64", ["v[0:7]", "v[8:9]", "v[10:11]", "v[0:7]"]),
           (8, "s_cbranch_vccnz", ["1"]),           # to 8 + 4 + 4 * 1 = 16: skips the store
           (12, "buffer_store_dwordx4", ["v[0:3]", "v4", "s[0:3]", "0", "offen"]),
           (16, "ds_read_b64", ["v[0:1]", "v2"]),   # the label
           (20, "s_cbranch_scc1", ["65530"])]       # back to 20 + 4 - 4 * 6 = 0
    first, last = kr.pair_loop(ins)
    assert (first, last) == (0, 5)
    regs = kr.regions(ins, first, last)
    assert [r["end_by"] for r in regs] == ["s_cbranch_vccnz", "label", "s_cbranch_scc1"]
    assert [r["events"] for r in regs] == ["M", "S", "d"]
