"""CPU tier: the scan for bzip2 marks (csrc/bzip2_scan.h) on the host emulation, and the host index (swc_index_blocks kind 10), each
held to the statement of the mark rule in tests/_bzip2_marks_cases.py -- never to each other.  All three thread orders."""
import bz2
import struct

import pytest

import _bzip2_build as B
import _bzip2_marks_cases as K
import _emu
import _emu_bzip2_marks as E
import swcompression_amd as swc
from swcompression_amd import corpus

ORDERS = (0, 1, 2)
CASES = K.all_cases(E.TILE)
WANT = {name: K.rule(b) for name, b in CASES}


@pytest.fixture(autouse=True)
def _forward_again():
    yield
    E.set_order(0)


def check(name, b, residue, cap=None, want=None):
    want = WANT[name] if want is None else want
    cap = len(want) + 1 if cap is None else cap
    n, refs = E.index(b, cap, residue)
    assert n == len(want), (name, residue, cap)
    assert refs == want[:cap], (name, residue, cap)


def test_the_cases_are_what_they_are_meant_to_be():
    """The case list hits the outcomes its names promise -- by the rule itself."""
    w = WANT
    assert E.TILE % 1024 == 0 and 1024 <= E.TILE <= 65536
    assert w["length 0"] == [] and w["length 13"] == [] and w["magic at bit 31"] == []
    assert w["length 14, mark at bit 32"] == [(32, 80, 0, 0xC0DE0000 ^ 32, 0)]
    assert [r[0] for r in w["end magic at bit 31, a mark behind"]] == [8 * 40 - 83]
    for name, b in CASES:
        if name.startswith("mark ends with the buffer"):
            assert w[name][-1][0] == 8 * len(b) - 80 and w[name][-1][1] == 80, name
        if name.startswith("one bit too late"):
            assert w[name] == [], name
        if name.startswith("last mark at bit"):
            assert len(w[name]) == 1 and w[name][0][0] % 8 == int(name.split()[4]), name
    both = w["every alignment, both magics"]
    assert sorted((r[0] % 8, r[4]) for r in both) == sorted((s, f) for s in range(8) for f in (0, 1))
    for name, border in (("chunk borders", 16), ("step borders", 1024), ("tile borders", E.TILE)):
        got = {(r[0] % 8, -(r[0] // 8) % border) for r in w[name]}
        assert got == {(s, d) for s in range(8) for d in (1, 3, 6)}, name
    assert [r[0] for r in w["80 bits apart"]] == [35, 115, 806, 886] and w["80 bits apart"][2][4:] == (0,) and w["80 bits apart"][3][4] == 1
    assert [(r[0], r[4], r[3]) for r in w["a block, then the end"]] == [(32, 0, 0x12345678), (8 * 4321 + 5, 1, 0x12345678)]
    assert [r[0] for r in w["the first test alone is met"]] == [16003]
    many = w["more than 64 tiles"]
    assert len(many) == 9 and {r[0] // 8 // E.TILE for r in many} == {0, 2, 63, 64, 65, 69, 70} and len(CASES[-3][1]) > 64 * E.TILE
    assert w["a megabyte of noise"] == []
    assert len(w["bare marks, 80 bits apart"]) == 300 and all(r[1] == 80 for r in w["bare marks, 80 bits apart"])


@pytest.mark.parametrize("order", ORDERS)
def test_every_case_at_every_residue(order):
    """The buffer at all 16 residues between guards, the refs between guards, workspace and *n pre-filled."""
    E.set_order(order)
    for name, b in CASES:
        for residue in range(16):
            check(name, b, residue)


@pytest.mark.parametrize("order", ORDERS)
def test_cap_contract(order):
    """cap 0, 1, n - 1, n, n + 5: the same *n, refs[0 .. min) those of the unlimited call -- the last one too -- and nothing behind."""
    E.set_order(order)
    for name in K.CAP_CASES:
        b = dict(CASES)[name]
        n = len(WANT[name])
        assert n >= 2
        for cap in K.caps(n):
            check(name, b, 9, cap=cap)
            got_n, refs = E.index(b, cap, 2, room=cap + 3)   # room behind the cap: still untouched
            assert (got_n, refs) == (n, WANT[name][:cap])


def test_host_index_kind_10():
    """swc_index_blocks kind 10 (no device) equals the rule on the same cases."""
    for name, b in CASES:
        assert swc.index_blocks("bzip2_marks", b, flags=True) == WANT[name], name
    b = dict(CASES)["80 bits apart"]
    assert swc.index_blocks("bzip2_marks", b) == [r[:4] for r in WANT["80 bits apart"]]


def test_block_marks_are_the_kind_5_refs_that_have_their_80_bits():
    for name, b in CASES:
        five = swc.index_blocks("bzip2", b, flags=True)
        assert [r[0] for r in five if r[0] + 80 <= 8 * len(b)] == [r[0] for r in WANT[name] if r[4] == 0], name
        assert all(r[1:] == (0, 0, 0, 0) for r in five), name


def _streams():
    text = corpus.p_text(450000, 31)
    one = bz2.compress(text, 1)
    return [("450 kB at level 1", one), ("streams back to back", bz2.compress(text[:70000], 1) + bz2.compress(text[70000:200000], 1) +
                                          bz2.compress(b"", 9) + bz2.compress(text[200000:230000], 9))] + list(B.multi_cases())


N_STREAMS = 4   # (the parametrisation below; _streams() is built inside the tests, and held to this)


@pytest.mark.parametrize("k", range(N_STREAMS))
def test_real_streams(k):
    """The marks of a real file are where the model's sequential walk arrives: block by block, end by end, each with its word."""
    streams = _streams()
    assert len(streams) == N_STREAMS, "a stream was added: N_STREAMS has to follow"
    name, data = streams[k]
    walked = K.walked_marks(data)
    assert len(walked) >= 4, name
    want = K.rule(data)
    assert [(r[0], r[4], r[3]) for r in want] == walked, name   # (no magic in the data of these files)
    assert swc.index_blocks("bzip2_marks", data, flags=True) == want, name
    for order in ORDERS:
        E.set_order(order)
        check(name, data, (5 * k + order) % 16, want=want)


def test_sanitizer_program(tmp_path):
    """The case list once through the stand-alone program (address and undefined-behaviour sanitizers; nothing loaded into python): every
    buffer ends where its allocation ends, the refs are an allocation of exactly what is to be written."""
    blob = []
    for i, (name, b) in enumerate(CASES):
        want = WANT[name]
        caps = (len(want) + 1,) if i % 7 else (len(want) + 1, max(len(want) - 1, 0), 1)
        for cap in caps:
            blob.append(struct.pack("<III", (i * 5 + cap) % 16, cap, len(b)) + b + struct.pack("<I", len(want)) + K.pack_refs(want[:cap]))
    out = _emu.run_program(tmp_path, E.SRC, E.MAIN, struct.pack("<I", len(blob)) + b"".join(blob))
    assert "%d cases in 3 orders, 0 mismatches" % len(blob) in out
