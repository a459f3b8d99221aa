"""Every argument error of the 19 solving and creating entry points is the one
the parent commit reported (tests/golden/abi_errors.json, written by
tests/golden/make_abi_errors.py from the parent's library), and two errors at
once give one of the two, never a success and never TRITD_ERR_NODEV: every
argument check still comes before the first HIP call.

Without a visible GPU every mutation is called and an accepted one ends at the
missing device.  With one, only the refused mutations are called, so nothing
is computed or created on the device."""
import json
import os

import pytest

import abi_error_cases as cases
from conftest import GOLDEN
from tritd import _lib

with open(os.path.join(GOLDEN, "abi_errors.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def bufs():
    return cases.Buffers()


def test_the_fixture_covers_every_entry_point_and_mutation():
    assert set(RECORDED["entry_points"]) == set(cases.ENTRY_POINTS) and len(cases.ENTRY_POINTS) == 19
    for entry, rec in RECORDED["entry_points"].items():
        assert len(cases.names(entry)) == len(_lib.SIGNATURES[entry][1]), entry
        assert list(rec["single"]) == [m[0] for m in cases.mutations(entry)], entry


@pytest.mark.parametrize("entry", list(cases.ENTRY_POINTS))
def test_single_mutations_answer_as_the_parent_did(bufs, entry):
    rec = RECORDED["entry_points"][entry]["single"]
    gpu = _lib.device_count() > 0
    for name, changes in cases.mutations(entry):
        if rec[name] == "accepted":
            if not gpu:
                assert cases.call(_lib.lib, bufs, entry, changes)[0] == cases.NODEV, name
            continue
        assert list(cases.call(_lib.lib, bufs, entry, changes)) == rec[name], name


@pytest.mark.parametrize("entry", list(cases.ENTRY_POINTS))
def test_two_refused_mutations_give_one_of_their_answers(bufs, entry, record_property):
    rec = RECORDED["entry_points"][entry]
    muts = dict(cases.mutations(entry))
    changed = pairs = 0
    for x, a in enumerate(rec["refused"]):
        for b, parent in zip(rec["refused"][x + 1:], rec["winners"][x]):
            if parent in ".x":  # not combinable / excluded by name in the generator
                continue
            got = list(cases.call(_lib.lib, bufs, entry, muts[a] + muts[b]))
            assert got[0] not in (0, cases.NODEV), (a, b, got)
            assert got in (rec["single"][a], rec["single"][b]), (a, b, got)
            pairs += 1
            if parent != "=":
                changed += got != rec["single"][a if parent == "1" else b]
    # (reported, not asserted: which of two errors wins is not part of the ABI)
    record_property("pairs", pairs)
    record_property("winner_changed", changed)
    print("%s: %d pairs, %d changed winner against the parent" % (entry, pairs, changed))
