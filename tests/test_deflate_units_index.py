"""CPU tier: the unit index of a raw Deflate stream (swc_index_blocks kind 3) against a Python restatement of its rule, and the
checksum combiners (swc_crc32_combine, swc_adler32_combine) against zlib.  No device is needed."""
import random
import zlib

import pytest

import swcompression_amd as swc
from swcompression_amd import _lib

MARK = b"\x00\x00\xff\xff"
JOINED, OPEN = 1, 2
DEFAULT_UNIT_BYTES = 0     # the library ships with the cut switched off


def rule(data, unit_bytes):
    """The index rule restated: a cut behind every marker; a cut stands when the unit it closes holds at least unit_bytes; no cut
    at the very end; 0 = never cut.  Returns [(offset, comp_len, 0, aux)]."""
    cuts, start, i = [], 0, 0
    if unit_bytes:
        while True:
            i = data.find(MARK, i)
            if i < 0:
                break
            cut = i + 4
            if cut < len(data) and cut - start >= unit_bytes:
                cuts.append(cut)
                start = cut
            i += 1
    edges = [0] + cuts + [len(data)]
    n = len(edges) - 1
    return [(edges[k], edges[k + 1] - edges[k], 0, (JOINED if k else 0) | (OPEN if k + 1 < n else 0)) for k in range(n)]


@pytest.fixture
def knob():
    lib = _lib.load()

    def set_(v):
        assert lib.swc_set_tuning(b"deflate_unit_bytes", v) == 0
    yield set_
    lib.swc_set_tuning(b"deflate_unit_bytes", DEFAULT_UNIT_BYTES)


def planted(rnd, n, marks):
    d = bytearray(rnd.getrandbits(8) for _ in range(n))
    for m in marks:
        d[m:m + 4] = MARK
    return bytes(d[:n])


@pytest.mark.parametrize("unit_bytes", [1, 100, 32768])
def test_index_matches_the_rule(knob, unit_bytes):
    rnd = random.Random(unit_bytes)
    n = 200000
    cases = {
        "planted": planted(rnd, n, [0, 50, 99, 100, 104, 4000, 36000, 36004, 70000, 140000, n - 5]),
        "marker at the end": planted(rnd, n, [40000, n - 4]),
        "only at the end": planted(rnd, 1000, [996]),
        "no marker": bytes(b | 1 for b in planted(rnd, 50000, [])),
        "overlapping": b"\x00" * 7 + b"\xff" * 5 + b"\x00\x00\x00\xff\xff\xff\x00\x00\xff\xff" + b"\x01" * 50,
        "all markers": MARK * 300,
        "few symbols": bytes(rnd.choice(b"\x00\xff") for _ in range(60000)),
        "short": b"\x00\x00\xff",
        "a marker alone": MARK,
        "empty": b"",
        "closing empty block": planted(rnd, 80000, [33000]) + b"\x01" + MARK,
    }
    knob(unit_bytes)
    for name, data in cases.items():
        assert swc.index_blocks("deflate", data) == rule(data, unit_bytes), name
    want = rule(cases["planted"], unit_bytes)
    assert len(want) == {1: 11, 100: 7, 32768: 5}[unit_bytes]
    assert all(r[1] >= unit_bytes for r in want[:-1])
    assert rule(cases["marker at the end"], unit_bytes)[-1][0] == 40004     # the cut at the very end is dropped
    assert len(rule(cases["closing empty block"], unit_bytes)) == 2


def test_knob_zero_never_cuts(knob):
    knob(0)
    data = planted(random.Random(5), 100000, [40000, 80000])
    assert swc.index_blocks("deflate", data) == [(0, len(data), 0, 0)]
    assert _lib.load().swc_set_tuning(b"deflate_unit_bytes", -1) != 0


def test_full_flush_units_are_found(knob):
    """A Z_FULL_FLUSH stream: every unit but the last ends with the marker, and the pieces are where zlib flushed."""
    knob(1)
    rnd = random.Random(11)
    parts = [bytes(rnd.choice(b"abcdefgh ") for _ in range(n)) for n in (5000, 1, 70000, 300)]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    pieces = [c.compress(p) + c.flush(zlib.Z_FULL_FLUSH) for p in parts[:-1]] + [c.compress(parts[-1]) + c.flush()]
    refs = swc.index_blocks("deflate", b"".join(pieces))
    assert [r[1] for r in refs] == [len(p) for p in pieces]
    assert [r[3] for r in refs] == [OPEN, JOINED | OPEN, JOINED | OPEN, JOINED]


def test_combine_against_zlib():
    lib = _lib.load()
    rnd = random.Random(3)
    data = bytes(rnd.getrandbits(8) for _ in range(70000))
    for cut in [0, 1, 15, 16, 17, 5551, 5552, 5553, 65520, 65521, 65522, 69999, 70000] + [rnd.randrange(70001) for _ in range(40)]:
        a, b = data[:cut], data[cut:]
        assert lib.swc_crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data), cut
        assert lib.swc_adler32_combine(zlib.adler32(a), zlib.adler32(b), len(b)) == zlib.adler32(data), cut
    # three pieces, folded left to right as the host folds the units of a run
    c = zlib.crc32(b"")
    ad = zlib.adler32(b"")
    for piece in (data[:100], b"", data[100:40000], data[40000:]):
        c = lib.swc_crc32_combine(c, zlib.crc32(piece), len(piece))
        ad = lib.swc_adler32_combine(ad, zlib.adler32(piece), len(piece))
    assert (c, ad) == (zlib.crc32(data), zlib.adler32(data))


def test_combine_beyond_4_gib():
    """len_b > 2^32: B = 2^32 + 12,345 zero bytes, whose sums come from combining halves (doubling); the one-step result must equal
    combining B's two parts one after the other."""
    lib = _lib.load()
    a = b"unit in front"
    block = bytes(1 << 20)
    c, ad, n = zlib.crc32(block), zlib.adler32(block), len(block)
    while n < 1 << 32:                                   # zeros ++ zeros, by the combiner itself: 2^20 -> 2^32
        c, ad, n = lib.swc_crc32_combine(c, c, n), lib.swc_adler32_combine(ad, ad, n), 2 * n
    tail = bytes(12345)
    ct, adt = zlib.crc32(tail), zlib.adler32(tail)
    cb, adb = lib.swc_crc32_combine(c, ct, len(tail)), lib.swc_adler32_combine(ad, adt, len(tail))   # sums of B
    lb = n + len(tail)
    assert lb > 1 << 32
    one_c = lib.swc_crc32_combine(zlib.crc32(a), cb, lb)
    one_a = lib.swc_adler32_combine(zlib.adler32(a), adb, lb)
    two_c = lib.swc_crc32_combine(lib.swc_crc32_combine(zlib.crc32(a), c, n), ct, len(tail))
    two_a = lib.swc_adler32_combine(lib.swc_adler32_combine(zlib.adler32(a), ad, n), adt, len(tail))
    assert (one_c, one_a) == (two_c, two_a)
    # and the doubling itself is right where zlib can still check it: 2^24 zeros
    c24, a24, m = zlib.crc32(block), zlib.adler32(block), len(block)
    while m < 1 << 24:
        c24, a24, m = lib.swc_crc32_combine(c24, c24, m), lib.swc_adler32_combine(a24, a24, m), 2 * m
    z = bytes(1 << 24)
    assert (c24, a24) == (zlib.crc32(z), zlib.adler32(z))
