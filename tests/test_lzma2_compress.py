"""LZMA2.compress / XZArchive.archive -- LZMA2 runs written on the device (SWC_CODEC_LZMA2_COMPRESS, csrc/lzma_comp.h).  An extension:
the reference has no LZMA encoder.

The contract: a unit is one run behind a dictionary reset -- chunks of exactly 65,536 bytes, each LZMA (lc 3, lp 0,
pb 2, distances up to 65,535) or stored, whichever is smaller, the controls by the table below, no packet across a chunk end,
a match at distance rep0 + 1 always in the rep0 form, an end marker unless the unit is a segment.  Every stream must decode under
liblzma and the oracle, be the same in every lane order, and come out of an INDEPENDENT range encoder (tests/_lzma_build.py) again
when that is fed the packets tests/_lzma_packets.py reads from it.
CPU tier: the kernel source on the host emulation (tests/host_emu/emu_lzma_comp.cpp, through tests/_emu_lzma_comp.py)."""
import ctypes as C
import functools
import json
import lzma
import os
import random
import struct

import pytest

import _emu
import _emu_lzma_comp as E
import _lzma_build as B
import _lzma_packets as P
import _oracle as O
import swcompression_amd as swc
from swcompression_amd import _lib, corpus

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ref_inline_vectors.json")))
GOLD_INPUTS = [s.encode("latin1") for s in GOLD["roundtrip_strings"]] + [bytes.fromhex(h) for h in GOLD["roundtrip_bytes"]]
DB, CHUNK = E.DICT_BYTE, E.CHUNK
_P7 = (b"periodx" * 9400)[:65536 + 200]                       # a period of 7 across byte 65,536
TRT = corpus.p_text(65536, 31) + corpus.p_rand(65536, 32) + corpus.p_text(65536, 33)
RT = corpus.p_rand(65536, 34) + corpus.p_text(65536, 35)

# name -> input: the edge sizes, every side of a chunk's end, every kind of content, mixed units, a period across a cut
INPUTS = dict(
    [("empty", b"")] + [("n%d" % n, corpus.p_text(n, 20 + n)) for n in (1, 2, 15, 16, 17)]
    + [("text65535", corpus.p_text(65535, 1)), ("text65536", corpus.p_text(65536, 2)), ("text65537", corpus.p_text(65537, 3)),
       ("mix131073", corpus.p_mix(131073, 4)), ("rand70000", corpus.p_rand(70000, 5)), ("zeros200000", bytes(200000)),
       ("bytes256", bytes(range(256))), ("bin100000", corpus.p_bin(100000, 6)), ("text_rand_text", TRT), ("rand_text", RT),
       ("period7", _P7)]
    + [("gold%d" % i, g) for i, g in enumerate(GOLD_INPUTS)])
NAMES = list(INPUTS)
TEXT_NAMES = [n for n in NAMES if n.startswith("text6")]


def liblzma_raw(stream):
    """The plain bytes of a raw LZMA2 stream under liblzma with a dictionary of 65,536 bytes; the stream must end at its end marker."""
    d = lzma.LZMADecompressor(lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": 65536}])
    out = d.decompress(stream)
    assert d.eof and not d.unused_data
    return out


def liblzma_preset0(data):
    return lzma.compress(data, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": 0, "dict_size": 65536}])


@functools.lru_cache(maxsize=None)
def compressed(order=0):
    """name -> the run of every input, thread order `order` of the emulated regions."""
    E.set_order(order)
    try:
        res = E.compress([INPUTS[n] for n in NAMES])
    finally:
        E.set_order(0)
    for n, (st, z, cons, zl) in zip(NAMES, res):
        assert st == 0 and zl == len(z) and cons == len(INPUTS[n]), (n, st, zl, cons)
    return {n: r[1] for n, r in zip(NAMES, res)}


@functools.lru_cache(maxsize=None)
def parsed(name):
    chunks, plain, used, marked = P.parse(compressed()[name])
    assert plain == INPUTS[name] and used == len(compressed()[name]) and marked
    return chunks


def test_bound_is_the_documented_formula():
    for n in (0, 1, 65535, 65536, 65537, 131072, 1 << 20, (1 << 20) + 1):
        assert E.lib.emu_lzma2_compress_bound(n) == E.bound(n) == n + 3 * -(-n // 65536) + 1


@pytest.mark.parametrize("order", [0, 1, 2], ids=["forward", "reverse", "shuffled"])
def test_round_trip_under_liblzma_and_the_oracle_in_every_lane_order(order):
    z0, zs = compressed(0), compressed(order)
    for n in NAMES:
        z, x = zs[n], INPUTS[n]
        assert z == z0[n], "the stream of %s depends on the order of the lanes" % n
        assert len(z) <= E.bound(len(x))
        if order == 0:
            assert liblzma_raw(z) == x, n
            st, out, used = O.lzma2(z, DB)
            assert (st, out, used) == (0, x, len(z)), (n, st, used, len(z))


@pytest.mark.parametrize("name", NAMES)
def test_replay_through_an_independent_encoder_gives_the_same_bytes(name):
    """The controls and packets read back from the stream, written again by the builder's range encoder and model: carry, flush
    and every cell update of the kernel against an encoder that shares no code with it."""
    b = B.Builder("lzma2", dict_byte=DB, auto_split=False)
    x = INPUTS[name]
    for c in parsed(name):
        if c.comp is None:
            b.stored(x[c.start:c.start + c.unpack], reset_dict=c.control == 1)
            continue
        b.chunk(c.control, props=c.props)
        for p in c.packets:
            if p.kind == "literal":
                b.literal(p.byte)
            elif p.kind == "match":
                b.match(p.distance, p.length)
            else:
                assert p.kind == "rep0"
                b.rep(0, p.length)
    case = b.case(name)
    assert case.plain == x and case.status == 0
    assert case.stream == compressed()[name]
    assert case.liblzma_ok


@pytest.mark.parametrize("name", NAMES)
def test_contract_of_chunks_and_packets(name):
    x, z, chunks = INPUTS[name], compressed()[name], parsed(name)
    assert len(chunks) == -(-len(x) // CHUNK)
    prev = None
    for k, c in enumerate(chunks):
        assert c.start == k * CHUNK and c.unpack == min(CHUNK, len(x) - c.start)       # every u 65,536 but the last
        if c.comp is None:
            assert c.control == (1 if k == 0 else 2)
        else:
            want = 0xE0 if k == 0 else 0xC0 if prev.comp is None else 0x80
            assert c.control == want, (k, hex(c.control))
            assert c.props == ((3, 0, 2) if want != 0x80 else None)
            assert (6 if c.props else 5) + c.comp < 3 + c.unpack                        # the LZMA form only where it is smaller
            at = c.start
            for p in c.packets:                                                         # (P.parse asserts: none crosses the chunk's end)
                assert p.pos == at
                at += p.length
                assert p.kind in ("literal", "match", "rep0")
                if p.kind != "literal":
                    assert 2 <= p.length <= 273 and 1 <= p.distance <= 65535 and p.distance <= p.pos
                if p.kind == "match":
                    assert p.distance != p.rep0 + 1, "a plain match at distance rep0 + 1"
                if p.kind == "rep0":
                    assert p.distance == p.rep0 + 1
            assert at == c.start + c.unpack
        prev = c
    assert z[-1] == 0


def test_controls_of_mixed_units_and_sizes():
    assert [c.control for c in parsed("text_rand_text")] == [0xE0, 0x02, 0xC0]
    assert [c.control for c in parsed("rand_text")] == [0x01, 0xC0]
    assert len(compressed()["rand70000"]) == E.bound(70000)                             # incompressible: exactly the bound
    assert compressed()["empty"] == b"\0"
    for n in TEXT_NAMES:
        # LZMA chunks only -- but for the one-byte chunk of the 65,537-byte unit: header 5 + a flush of 5 is never below 3 + u for
        # u < 8, so by the contract's own rule such a chunk is stored
        assert all(c.comp is not None or c.unpack < 8 for c in parsed(n)) and len(compressed()[n]) < len(INPUTS[n])
    assert [c.control for c in parsed("text65537")] == [0xE0, 0x02]
    kinds = [p.kind for c in parsed("bin100000") for p in c.packets]
    assert kinds.count("rep0") >= 1
    # the match that the chunk's end cut goes on behind it, in the model that chunk left
    c1 = parsed("period7")[1]
    assert c1.control == 0x80 and len(c1.packets) == 1 and c1.packets[0].kind in ("match", "rep0")
    assert c1.packets[0].distance % 7 == 0 and c1.packets[0].length == 200
    assert parsed("period7")[0].packets[-1].kind in ("match", "rep0")
    assert parsed("period7")[0].packets[-1].pos + parsed("period7")[0].packets[-1].length == CHUNK


# measured on the emulation: the runs of five 64 KiB text units are 1.0607 x liblzma's preset 0 with the same dictionary
SIZE_QUOTIENT = 1.0607


def test_size_against_liblzma_preset_0():
    """A guard against a broken parse, not a target: two points of margin on the measured quotient."""
    xs = [corpus.p_text(65536, s) for s in range(11, 16)]
    ours = sum(len(r[1]) for r in E.compress(xs))
    theirs = sum(len(liblzma_preset0(x)) for x in xs)
    print("lzma2_compress %d bytes, liblzma preset 0 %d bytes: quotient %.4f" % (ours, theirs, ours / theirs))
    assert ours / theirs <= SIZE_QUOTIENT + 0.02


CAPACITY_NAMES = ["text65537", "rand70000", "n17", "text_rand_text", "zeros200000", "n1"]


def test_capacity_reports_the_size_and_writes_nothing_past_it():
    for order in (0, 1, 2):
        E.set_order(order)
        try:
            xs = [INPUTS[n] for n in CAPACITY_NAMES]
            sizes = [len(compressed()[n]) for n in CAPACITY_NAMES]
            for cut in (7, 1):
                caps = [max(s - cut, 0) for s in sizes]
                for n, s, cap, (st, z, cons, zl) in zip(CAPACITY_NAMES, sizes, caps, E.compress(xs, caps=caps)):   # (exact=True: the guards)
                    assert st == 901 and zl == s and cons == len(INPUTS[n]), (n, st, zl, s)
                    assert z == compressed()[n][:cap], n                                # what is there is the run's beginning
            for n, s, (st, z, _, zl) in zip(CAPACITY_NAMES, sizes, E.compress(xs, caps=sizes)):     # exactly enough room
                assert st == 0 and z == compressed()[n]
        finally:
            E.set_order(0)


def segments():
    """30 segments.  A reader that counts positions from the start of the stream (the reference) and one that counts from the last
    dictionary reset (liblzma) agree on pos_state only where a reset falls on a multiple of 4, so the segments that an odd-sized
    one pushes off such a boundary are incompressible and come out stored: then both read the same bytes."""
    rnd = random.Random(9)
    segs = [corpus.p_text(70000, 1), b"", b"a", corpus.p_rand(3, 2), corpus.p_rand(12, 3), corpus.p_text(4096, 4), b"",
            corpus.p_mix(65536 + 16, 5), b"x", corpus.p_rand(15, 6), corpus.p_text(1600, 7), bytes(200000), corpus.p_bin(3200, 8)]
    while len(segs) < 29:
        segs += [corpus.p_text(16 * rnd.randint(1, 40), 40 + len(segs))] if rnd.random() < 0.6 else [b"q", corpus.p_rand(15, len(segs))]
    return segs[:29] + [corpus.p_text(5000, 99)]


def test_segments_of_a_longer_stream_join_into_one():
    segs = segments()
    assert len(segs) == 30 and b"" in segs and any(len(s) == 1 for s in segs)
    aux = [E.SEGMENT] * 29 + [0]
    res = E.compress(segs, aux=aux)
    stream, offs, at = b"", [], 0
    for s, a, (st, z, cons, zl) in zip(segs, aux, res):
        assert st == 0 and zl == len(z) <= E.bound(len(s)) - a and cons == len(s)
        chunks, plain, used, marked = P.parse(z)
        assert plain == s and used == len(z) and marked == (a == 0)
        assert s or z == b""                                                            # an empty segment is nothing at all
        assert all(c.comp is None for c in chunks) or at % 4 == 0, "an LZMA chunk behind a reset off a multiple of 4"
        if s and at % 16 == 0:
            offs.append(at)
        stream += z
        at += len(s)
    plain = b"".join(segs)
    assert liblzma_raw(stream) == plain
    st, out, used = O.lzma2(stream, DB)
    assert (st, out, used) == (0, plain, len(stream))
    # swc_index_blocks kind 8: the units are exactly the non-empty segments that begin at a multiple of 16
    lib = _lib.load()
    assert lib.swc_set_tuning(b"lzma2_run_bytes", 1) == 0
    try:
        refs = swc.index_blocks("lzma2_runs", bytes([DB]) + stream, flags=True)
    finally:
        lib.swc_set_tuning(b"lzma2_run_bytes", 0)
    got, p = [], 0
    for off, comp, uncomp, a, _ in refs:
        got.append(p)
        p += uncomp
    assert got == offs and p == len(plain) and len(offs) >= 12


def _case_file(cases):
    blob = struct.pack("<I", len(cases))
    for x, cap, aux, order in cases:
        blob += struct.pack("<IIII", cap, aux, order, len(x)) + x
    return blob


def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """The emulation as a program of its own under the address and undefined-behaviour sanitizers (nothing is loaded into python):
    every input and output ends with its allocation.  Edge inputs in the three lane orders, the capacity cases, segments."""
    names = ["empty", "n1", "n2", "n15", "n16", "n17", "text65535", "text65537", "rand70000", "bytes256", "rand_text", "period7", "gold8"]
    cases, want = [], []
    for order in (0, 1, 2):
        for n in names:
            z = compressed()[n]
            cases.append((INPUTS[n], E.bound(len(INPUTS[n])), 0, order))
            want.append((0, len(z), z))
    for n in CAPACITY_NAMES:
        z = compressed()[n]
        for cap in (len(z) - 7 if len(z) >= 7 else 0, len(z) - 1, 0, len(z)):
            cases.append((INPUTS[n], cap, 0, 1))
            want.append((0 if cap >= len(z) else 901, len(z), z[:cap] if cap >= len(z) else None))
    for n in ("n16", "text65537", "empty"):
        z = compressed()[n]
        cases.append((INPUTS[n], len(z) - 1, E.SEGMENT, 2))
        want.append((0, len(z) - 1, z[:-1]))
    out = _emu.run_program(tmp_path, E.SRC, E.MAIN, _case_file(cases))
    lines = [l.split() for l in out.strip().splitlines()]
    assert len(lines) == len(cases), out[-2000:]
    for k, (l, (st, zl, z)) in enumerate(zip(lines, want)):
        assert (int(l[0]), int(l[1]), int(l[2])) == (k, st, zl), (k, l, st, zl)
        if z is not None:
            s = 0
            for b in z:
                s = (s * 131 + b) & 0xFFFFFFFFFFFF
            assert int(l[3]) == s, k


def test_entry_points_without_a_device_and_their_arguments():
    lib = _lib.load()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t()
    x = b"abcabcabc" * 10
    # the empty archive has no block: answered without a device
    a = swc.XZArchive.archive(b"")
    assert len(a) == 32 and lzma.decompress(a) == b"" and O.xz_unarchive(a) == (0, b"")
    for check in ("none", "crc32", "crc64", "sha256"):
        a = swc.XZArchive.archive(b"", check=check)
        assert len(a) == 32 and lzma.decompress(a) == b"" and O.xz_unarchive(a) == (0, b"")
    for check_type in (2, 3, 5, 9, 11, -1):
        assert lib.swc_xz_archive(x, len(x), check_type, 0, C.byref(out), C.byref(n)) == 903
    for block_size in (1, 4095, 4096 + 8, (1 << 30) + 16):
        assert lib.swc_xz_archive(x, len(x), 4, block_size, C.byref(out), C.byref(n)) == 903
    assert lib.swc_xz_archive(x, len(x), 4, 0, None, C.byref(n)) == 903
    assert lib.swc_lzma2_compress(x, len(x), None, C.byref(n)) == 903
    from swcompression_amd.batch import CODECS
    assert CODECS["lzma2_compress"] == 10 and lib.swc_batch_workspace_bytes(10, 100, 1 << 20) == 0
    if swc.device_available():
        return                                                                          # (the gpu tier has the rest)
    assert lib.swc_lzma2_compress(x, len(x), C.byref(out), C.byref(n)) == 902
    assert lib.swc_lzma2_compress(b"", 0, C.byref(out), C.byref(n)) == 902
    for check_type in (0, 1, 4, 10):
        assert lib.swc_xz_archive(x, len(x), check_type, 0, C.byref(out), C.byref(n)) == 902
        assert lib.swc_xz_archive(x, len(x), check_type, 4096, C.byref(out), C.byref(n)) == 902
    with pytest.raises(swc.DeviceError):
        swc.LZMA2.compress(x)
    with pytest.raises(swc.DeviceError):
        swc.XZArchive.archive(x)
