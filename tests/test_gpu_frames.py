"""GPU tier of the container layer: every archive of tests/_frames_cases.py through the engine, held to the expectation stated by hand
from the reference's Swift -- status, the bytes a result or an error carries, the parts of the multi calls.  The reference is strictly
serial; the engine discovers LZ4 blocks first, takes .xz blocks from the index at the end of the file, finds bzip2 blocks by their
marks, cuts gzip members and LZMA2 data into units and decodes whole sets of archives in one launch.  An archive with two faults
shows whether it still answers as the reference would.  Everything runs twice: with the tuning values as shipped, and with every
value that adds another way to reorder switched on."""
import contextlib
import random

import pytest

import _frames_cases as FC
import swcompression_amd as swc
from swcompression_amd import _lib

pytestmark = pytest.mark.gpu

KINDS = list(FC.KINDS)
CUT = {"deflate_unit_bytes": 1024, "deflate_units_linked": 1, "lzma2_run_bytes": 4096, "gzip_member_scan": 1, "bzip2_scan_bytes": 1}
GROWS = {"gzip": b"gzip_scan_members", "xz": b"lzma2_run_units", "bzip2": b"bzip2_scan_marks"}   # swc_stat: the cut paths were taken


@contextlib.contextmanager
def knobs(cut):
    """The tuning values of CUT for the body (cut) or as shipped (all 0); every one is 0 again afterwards, whatever happened."""
    lib = _lib.load()
    try:
        for key, v in CUT.items():
            assert lib.swc_set_tuning(key.encode(), v if cut else 0) == 0, key
        yield lib
    finally:
        for key in CUT:
            lib.swc_set_tuning(key.encode(), 0)


def _stat(lib, kind):
    return lib.swc_stat(GROWS[kind]) if kind in GROWS else 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cut", [False, True], ids=["as-shipped", "cut"])
def test_single_shot_and_multi_calls(cut, kind):
    """Every case through its single-shot call and, where the container has one, its multi call, through the Python mirror (so the
    error's class, .case and .data are checked too)."""
    wrong = []
    with knobs(cut) as lib:
        before = _stat(lib, kind)
        for c in FC.KINDS[kind]():
            got = FC.engine_single(c)
            if got != (c.status, c.out):
                wrong.append((c.name, "single", got[0], len(got[1]), "stated", c.status, len(c.out), c.source))
            if c.parts is not None:
                got = FC.engine_multi(c)
                if got != (c.multi_status, c.parts):
                    wrong.append((c.name, "multi", got[0], [len(p) for p in got[1]], "stated", c.multi_status, [len(p) for p in c.parts], c.source))
        grown = _stat(lib, kind) - before
    assert not wrong, wrong
    if cut and kind in GROWS:
        assert grown > 0, "%s did not grow: the cut variant has tested nothing" % GROWS[kind].decode()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cut", [False, True], ids=["as-shipped", "cut"])
def test_whole_sets_in_one_launch(cut, kind):
    """All cases of a kind in ONE swc_unarchive_many call, in order, in a seeded shuffle, and over a device list: each archive's
    (status, data) is the stated one whatever its neighbours are.  (The call takes no dictionary: the LZ4 cases that need one stay out.)"""
    cases = [c for c in FC.KINDS[kind]() if c.dictionary is None]
    assert len(cases) >= 40
    shuffled = list(cases)
    random.Random(0xF4A3E5).shuffle(shuffled)
    with knobs(cut) as lib:
        before = _stat(lib, kind)
        for order, devices in ((cases, None), (shuffled, None), (cases, [0])):
            got = swc.unarchive_many(kind, [c.data for c in order], devices=devices)
            wrong = [(c.name, st, len(data), "stated", c.status, len(c.out), c.source) for c, (st, data) in zip(order, got) if (st, data) != (c.status, c.out)]
            assert len(got) == len(order) and not wrong, wrong
        grown = _stat(lib, kind) - before
    if cut and kind in ("xz", "bzip2"):
        assert grown > 0, "%s did not grow: the cut variant has tested nothing" % GROWS[kind].decode()
