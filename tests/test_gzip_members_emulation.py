"""CPU tier: the scan for plain gzip members (csrc/gzip_scan.h) on the host emulation, and the host index (swc_index_blocks kind 9),
each held to the statement of the candidate rule in tests/_gzip_members_cases.py -- never to each other.  All three thread orders."""
import struct

import pytest

import _emu
import _emu_gzip_members as E
import _gzip_members_cases as K
import swcompression_amd as swc

ORDERS = (0, 1, 2)
CASES = K.all_cases(E.TILE)
WANT = {name: K.rule(b) for name, b in CASES}


@pytest.fixture(autouse=True)
def _forward_again():
    yield
    E.set_order(0)


def check(name, b, residue, cap=None):
    want = K.rule(b) if name is None else WANT[name]
    cap = len(want) + 1 if cap is None else cap
    n, refs = E.index(b, cap, residue)
    assert n == len(want), (name, residue, cap)
    assert refs == want[:cap], (name, residue, cap)


def test_tile_is_as_the_issue_bounds_it():
    assert E.TILE % 1024 == 0 and 1024 <= E.TILE <= 65536


@pytest.mark.parametrize("order", ORDERS)
def test_lengths_at_every_residue(order):
    """Lengths 0..44 and within 20 bytes of one and of two tiles, the buffer at all 16 residues between guards, the refs between guards."""
    E.set_order(order)
    for name, b in CASES:
        if name.startswith("length "):
            for residue in range(16):
                check(name, b, residue)


@pytest.mark.parametrize("order", ORDERS)
def test_the_last_candidate(order):
    """A candidate at exactly len - 20; the pattern at len - 19 is none."""
    E.set_order(order)
    for n in (20, 21, 39, 40, 1000, E.TILE - 3, E.TILE, E.TILE + 19, E.TILE + 20):
        b, late = K.of_length(n), K.of_length(n, late=True)
        assert K.rule(b)[-1][0] - K.rule(b)[-1][3] == n - 20
        assert late[n - 19:n - 16] == b"\x1f\x8b\x08" and all(r[0] - r[3] < n - 20 for r in K.rule(late))
        for residue in (0, 1, 7, 15):
            check(None, b, residue)
            check(None, late, residue)


@pytest.mark.parametrize("order", ORDERS)
def test_dense_candidates_and_soak(order):
    """1f 8b 08 repeated -- candidates three bytes apart -- and buffers over a nine-byte alphabet of 3 tiles + 37 bytes: candidates on every
    chunk, wave-step and tile border."""
    E.set_order(order)
    for name, b in CASES:
        if name.startswith(("dense ", "soak ")):
            assert len(WANT[name]) == max(0, (len(b) - 20) // 3 + 1) if name.startswith("dense") else len(WANT[name]) > 10
            for residue in (0, 5, 11) if len(b) > 5000 else range(16):
                check(name, b, residue)
    for seed in range(3, 8):
        b = K.soak(3 * E.TILE + 37, seed)
        check(None, b, (seed * 5) % 16)


@pytest.mark.parametrize("order", ORDERS)
def test_headers(order):
    E.set_order(order)
    names = sorted(K.header_cases())
    assert len([x for x in names if x.startswith("flags ")]) == 32
    for name in names:
        for residue in (0, 3, 13):
            check(name, dict(CASES)[name], residue)


def test_headers_are_what_they_are_meant_to_be():
    """The header cases hit the outcomes they are named for -- by the rule itself."""
    c = K.header_cases()
    r = {k: K.rule(v) for k, v in c.items()}
    for f in range(32):
        first = r["flags %02x" % f][0]
        assert first[4] == 0 and first[3] == 10 + (9 if f & 4 else 0) + (9 if f & 8 else 0) + (6 if f & 16 else 0) + (2 if f & 2 else 0)
    assert r["xlen past the end"][-1][4] == 1 and r["xlen to the last byte"][0][4] == 1
    for what in ("name", "comment"):
        assert r["%s of 255" % what][0][4] == 0 and r["%s of 256" % what][0][4] == 0 and r["%s of 257" % what][0][4] == 1
    assert len(r["name holds the magic"]) == 3 and r["name holds the magic"][0][4] == 1   # (the candidate in the name cuts the member short)
    assert len(r["name without a zero"]) > 150 and all(x[4] == 1 for x in r["name without a zero"])
    assert r["header ends behind the next"][0][4] == 1 and len(r["header ends behind the next"]) == 3
    assert r["next too close"][0] == (0, 0, 0, 0, 1)
    assert r["last at len - 20"] == [(43, 2, 0x88776655, 10, 0)] and r["none at len - 19"] == []
    assert r["isize words"][0][2] == 0x01020304 and r["isize words"][1][2] == 0xFFFFFFFF


@pytest.mark.parametrize("order", ORDERS)
def test_cap_contract(order):
    """cap 0, 1, n - 1, n, n + 1: the same *n, refs[0 .. min) those of the unlimited call -- the last one too -- and nothing behind."""
    E.set_order(order)
    for name in ("soak 0", "dense 1027", "flags 1f", "length %d" % (E.TILE + 7)):
        b = dict(CASES)[name]
        n = len(WANT[name])
        assert n >= 2
        for cap in (0, 1, n - 1, n, n + 1):
            check(name, b, 9, cap=cap)
            got_n, refs = E.index(b, cap, 2, room=cap + 3)   # room behind the cap: still untouched
            assert (got_n, refs) == (n, WANT[name][:cap])


def test_host_index_kind_9():
    """swc_index_blocks kind 9 (no device) equals the rule on the same cases."""
    for name, b in CASES:
        assert swc.index_blocks("gzip_members", b, flags=True) == WANT[name], name
    b = dict(CASES)["flags 1f"]
    assert swc.index_blocks("gzip_members", b) == [r[:4] for r in WANT["flags 1f"]]


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
