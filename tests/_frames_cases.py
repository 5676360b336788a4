"""Container cases with their expectations STATED BY HAND from the reference's Swift (Sources/ of tsolomko/SWCompression 4.9.0), not
computed by the oracle: the status, the bytes the call returns or the error carries, and the list of the multi call.  Each case cites
the line that decides it.  The engine, the oracle and this file are three readings of the same source; the tests hold each pair
against the other (tests/test_frames_build.py, tests/test_gpu_frames.py).  TEST INFRASTRUCTURE ONLY.

Case(name, kind, data, status, out, parts, stage, source, multi_status, dictionary, dict_id)
  kind          'gzip' | 'zlib' | 'lz4' | 'xz' | 'bzip2'
  status, out   of the single-shot call (GzipArchive.unarchive, ZlibArchive.unarchive, LZ4.decompress, XZArchive.unarchive,
                BZip2.decompress): out is the result, or what the error carries (b"" where it carries nothing)
  parts         of the multi call (multiUnarchive, multiDecompress, splitUnarchive): the result, or the list the error carries;
                None where the container has no multi call.  multi_status: its status where it is not `status`.
  stage         'header': the reference throws before it decodes any payload (no device is needed for the answer);
                'payload' / 'trailer': inside or behind a decode
  dictionary, dict_id   the arguments of LZ4.decompress(data:dictionary:dictionaryID:)
  data          bytes; where one call of a builder made the whole archive, a _frames_build.Built with the builder's .layout
The rule `ISIZE == count % 2^32` (GzipArchive.swift:95) is stated here and left untested: a payload of 2^32 bytes is out of scope."""
import bz2
import collections
import functools
import re
import struct
import zlib

import _frames_build as F
import _lz4_build as L4
import _xz_build as X
from swcompression_amd import corpus

Case = collections.namedtuple("Case", "name kind data status out parts stage source multi_status dictionary dict_id")

GZ_H, GZ_A, DEFL = "GzipHeader.swift", "GzipArchive.swift", "Deflate.swift"
ZL_H, ZL_A = "ZlibHeader.swift", "ZlibArchive.swift"
LZ = "LZ4.swift"
XS, XB, XA, MB = "XZStreamHeader.swift", "XZBlock.swift", "XZArchive.swift", "LittleEndianByteReader+XZ.swift"
BZ = "BZip2.swift"
TRAP = 900   # the reference reads past the end of its reader: a Swift runtime trap (include/swc_status.h)


def _case(cases, kind, name, data, status, out=b"", parts=Ellipsis, stage="payload", source="", multi_status=None, dictionary=None, dict_id=None):
    """parts left out: [out] for a success, [] for an error (the errors that carry a list say so)."""
    if parts is Ellipsis:
        parts = None if kind == "zlib" else ([bytes(out)] if status == 0 else [])
    assert source and stage in ("header", "payload", "trailer"), name
    assert not any(c.name == name for c in cases), name
    cases.append(Case(name, kind, data if isinstance(data, bytes) else bytes(data), status, bytes(out), parts, stage, source, status if multi_status is None else multi_status,
                      dictionary, dict_id))


P0, P1 = b"", b"a"
P100, P5000, P70001 = corpus.p_text(100, 1), corpus.p_text(5000, 2), corpus.p_text(70001, 3)
PA, PB, PC = corpus.p_text(300, 11), corpus.p_text(200, 12), corpus.p_text(100, 13)
PFLUSH = corpus.p_text(20000, 4)          # ten pieces of 2 KB between flush points
BAD_TYPE = b"\x07\x00"                    # BFINAL, BTYPE = 3: DeflateError.wrongBlockType (Deflate.swift:239)
BAD_STORED = b"\x01\x05\x00\x05\x00abcde"  # LEN & NLEN != 0: wrongUncompressedBlockLengths (Deflate.swift:57)


# ------------------------------------------------------------------------------------------------------------------------------ gzip
@functools.lru_cache(maxsize=None)
def gzip_cases():
    cases = []
    G = F.gzip_member
    def add(name, data, status, out=b"", **kw):
        _case(cases, "gzip", name, data, status, out, **kw)
    for p in (P0, P1, P100, P5000):
        add("valid-%d" % len(p), G(p), 0, p, source=GZ_A + ":98")
    add("valid-ftext-mtime-os", G(P100, ftext=True, mtime=0x5F5E1000, xfl=2, os=3), 0, P100, source=GZ_H + ":107")
    add("valid-all-four-optional-parts", G(P100, extra=[("A", "p", b"xyz"), (1, 2, b"")], name=b"file.txt", comment=b"hello", fhcrc=True, ftext=True),
        0, P100, source=GZ_H + ":111-198")
    # processMember's and the header's guards, from both sides
    add("archive-of-20-bytes", G(P0, body=b"\x03\x00"), 0, b"", source=GZ_A + ":83")
    add("archive-of-19-bytes", G(P0, body=b"\x03\x00", cut=19), 601, stage="header", source=GZ_A + ":83")
    add("header-of-10-bytes-alone", G(P0, cut=10), 601, stage="header", source=GZ_A + ":83")
    add("header-of-9-bytes-alone", G(P0, cut=9), 601, stage="header", source=GZ_A + ":83")
    add("empty-input", b"", 601, parts=[], multi_status=0, stage="header", source=GZ_A + ":83 (multiUnarchive: :67, no member at all)")
    add("magic-first-byte", G(P100, magic=b"\x1e\x8b"), 601, stage="header", source=GZ_H + ":75")
    add("magic-second-byte", G(P100, magic=b"\x1f\x8c"), 601, stage="header", source=GZ_H + ":75")
    add("method-7", G(P100, method=7), 602, stage="header", source=GZ_H + ":81")
    add("method-9", G(P100, method=9), 602, stage="header", source=GZ_H + ":81")
    add("magic-and-method-wrong", G(P100, magic=b"\x1f\x8c", method=9), 601, stage="header", source=GZ_H + ":75 before :81")
    for bit in (0x20, 0x40, 0x80):
        add("reserved-flag-%02x" % bit, G(P100, reserved=bit), 603, stage="header", source=GZ_H + ":87")
    add("method-and-reserved-flag", G(P100, method=9, reserved=0x80), 602, stage="header", source=GZ_H + ":81 before :87")
    add("reserved-flag-and-wrong-header-crc", G(P100, reserved=0x20, fhcrc=0x1234), 603, stage="header", source=GZ_H + ":87 before :196")
    # FEXTRA
    add("xlen-0", G(P100, extra=[], xlen=0), 601, stage="header", source=GZ_H + ":123")
    add("xlen-3", G(P100, extra=[], xlen=3), 601, stage="header", source=GZ_H + ":123")
    add("xlen-4", G(P100, extra=[("A", "B", b"")]), 0, P100, source=GZ_H + ":123")
    add("xlen-beyond-the-file", G(P1, extra=[("A", "B", b"")], xlen=60000), 601, stage="header", source=GZ_H + ":123")
    add("xlen-exactly-what-is-left", G(P0, extra=[("A", "B", b"0123")], body=b"", cut=20), 102, source=GZ_H + ":123 passes; " + DEFL + ":37")
    add("subfield-si2-0", G(P100, extra=[("A", 0, b"zz")]), 603, stage="header", source=GZ_H + ":131")
    add("second-subfield-si2-0", G(P100, extra=[("A", "B", b"zz"), ("C", 0, b"")]), 603, stage="header", source=GZ_H + ":131")
    add("subfield-one-byte-longer-than-xlen", G(P100, extra=[("A", "B", b"12345")], xlen=8), 601, stage="header", source=GZ_H + ":145")
    add("subfield-exactly-xlen", G(P100, extra=[("A", "B", b"12345")]), 0, P100, source=GZ_H + ":145")
    for k in (1, 2, 3):
        # the loop goes on while xlen > 0 and takes SI1, SI2 and LEN from the bytes behind the region; xlen - 4 < 0 <= LEN
        add("xlen-leaves-%d-identifiers-from-a-stored-block" % k, G(P100, extra=[("A", "B", b"xy")], xlen=6 + k, body=F.deflate_stored(P100)), 601,
            stage="header", source=GZ_H + ":125-145 (SI2 = 0x64)")
        add("xlen-leaves-%d-si2-0-behind-the-region" % k, G(P0, extra=[("A", "B", b"xy")], xlen=6 + k, body=b"\x03\x00"), 603,
            stage="header", source=GZ_H + ":125-131 (SI2 = the 0x00 of the body)")
        add("xlen-leaves-1-file-ends-%d-behind" % k, G(P0, extra=[("A", "B", b"xyz1234")], xlen=12, body=b"", crc=0x55555555, cut=23 + k), TRAP,
            stage="header", source=GZ_H + ":126-137 (byte() past the end)")
    add("xlen-leaves-1-si2-0-then-the-end", G(P0, extra=[("A", "B", b"xyz1234")], xlen=12, body=b"", crc=0x00000055, cut=25), 603,
        stage="header", source=GZ_H + ":131")
    # FNAME, FCOMMENT
    add("name-without-its-zero", G(P0, name=b"abcdefghijkl", name_terminated=False, body=b"", cut=22), 601, stage="header", source=GZ_H + ":162")
    add("comment-without-its-zero", G(P0, comment=b"abcdefghijkl", comment_terminated=False, body=b"", cut=22), 601, stage="header", source=GZ_H + ":178")
    add("name-ends-and-comment-without-its-zero", G(P0, name=b"abc", comment=b"defghijkl", comment_terminated=False, body=b"", cut=23), 601,
        stage="header", source=GZ_H + ":178")
    add("name-zero-is-the-last-byte", G(P0, name=b"abcdefghijk", cut=22), 102, source=DEFL + ":37 (no bits left)")
    add("empty-name-and-comment", G(P100, name=b"", comment=b""), 0, P100, source=GZ_H + ":166,182")
    # FHCRC
    add("fhcrc-right", G(P100, fhcrc=True), 0, P100, source=GZ_H + ":196")
    right = struct.unpack("<H", G(P100, name=b"n", fhcrc=True)[12:14])[0]
    add("fhcrc-right-behind-a-name", G(P100, name=b"n", fhcrc=right), 0, P100, source=GZ_H + ":196")
    add("fhcrc-wrong", G(P100, name=b"n", fhcrc=right ^ 1), 604, stage="header", source=GZ_H + ":196")
    add("fhcrc-wrong-high-byte", G(P100, name=b"n", fhcrc=right ^ 0x8000), 604, stage="header", source=GZ_H + ":196")
    add("fhcrc-of-the-header-without-the-name", G(P100, name=b"n", fhcrc=zlib.crc32(bytes(G(P100, name=b"n")[:10])) & 0xFFFF), 604,
        stage="header", source=GZ_H + ":196 (headerBytes holds every byte read)")
    add("fhcrc-cut-after-one-byte", G(P0, name=b"abcdefgh", fhcrc=True, cut=20), 601, stage="header", source=GZ_H + ":193")
    # the trailer
    add("trailer-of-7-bytes", G(P100, cut=-1), 601, stage="trailer", source=GZ_A + ":91")
    add("trailer-absent", G(P100, cut=-8), 601, stage="trailer", source=GZ_A + ":91")
    add("crc-wrong", G(P100, crc=0x12345678), 605, P100, parts=[P100], stage="trailer", source=GZ_A + ":99,44")
    add("isize-wrong", G(P100, isize=99), 606, stage="trailer", source=GZ_A + ":95")
    add("isize-and-crc-wrong", G(P100, crc=0x12345678, isize=101), 606, stage="trailer", source=GZ_A + ":95 before :99")
    add("deflate-error-and-short-trailer", G(P0, name=b"abcd", body=BAD_TYPE, cut=-4), 102, source=DEFL + ":239 before " + GZ_A + ":91")
    add("deflate-stored-lengths-and-wrong-crc", G(b"abcde", body=BAD_STORED, crc=1), 101, source=DEFL + ":57")
    add("garbage-behind-one-member", G(P100) + b"\xAA" * 5, 0, P100, parts=[], multi_status=601, stage="trailer", source=GZ_A + ":47 (one member); :83")
    # several members
    m = [G(PA), G(PB), G(PC)]
    add("three-members", m[0] + m[1] + m[2], 0, PA, parts=[PA, PB, PC], source=GZ_A + ":67-76")
    add("member-2-of-3-wrong-crc", m[0] + G(PB, crc=7) + m[2], 0, PA, parts=[PA, PB], multi_status=605, source=GZ_A + ":72-73")
    add("member-2-bad-header-member-3-wrong-crc", m[0] + G(PB, method=9) + G(PC, crc=7), 0, PA, parts=[], multi_status=602, source=GZ_H + ":81")
    add("member-2-wrong-crc-member-3-bad-header", m[0] + G(PB, crc=7) + G(PC, method=9), 0, PA, parts=[PA, PB], multi_status=605, source=GZ_A + ":72-73")
    add("member-2-wrong-isize", m[0] + G(PB, isize=1) + m[2], 0, PA, parts=[], multi_status=606, source=GZ_A + ":95")
    add("member-1-wrong-crc", G(PA, crc=7) + m[1], 605, PA, parts=[PA], source=GZ_A + ":44; :72-73")
    for k in range(1, 20):
        add("garbage-of-%d-behind-three-members" % k, m[0] + m[1] + m[2] + b"\xAA" * k, 0, PA, parts=[], multi_status=601, source=GZ_A + ":83")
    add("garbage-of-20-behind-three-members", m[0] + m[1] + m[2] + b"\xAA" * 20, 0, PA, parts=[], multi_status=601, source=GZ_H + ":75")
    mid = bytes(range(65, 91))
    add("member-ends-in-mid-byte-then-another", G(mid, body=F.deflate_mid_byte(mid)) + m[1], 0, mid, parts=[mid, PB], source=GZ_A + ":89")
    add("member-ends-in-mid-byte-wrong-isize", G(mid, body=F.deflate_mid_byte(mid), isize=27) + m[1], 606, parts=[], source=GZ_A + ":89,95")
    # members cut into units by "deflate_unit_bytes" (independent pieces, and pieces that share history)
    for tag, full in (("full-flush", True), ("sync-flush", False)):
        body = F.deflate_flushed(PFLUSH, full=full)
        add("flushed-member-%s" % tag, G(PFLUSH, body=body), 0, PFLUSH, source=GZ_A + ":98")
        add("flushed-member-%s-wrong-crc" % tag, G(PFLUSH, body=body, crc=5), 605, PFLUSH, parts=[PFLUSH], stage="trailer", source=GZ_A + ":99,44")
        add("flushed-member-%s-wrong-isize-and-crc" % tag, G(PFLUSH, body=body, crc=5, isize=19999), 606, stage="trailer", source=GZ_A + ":95")
        add("flushed-members-%s-second-wrong-crc" % tag, G(PFLUSH, body=body) + G(PFLUSH, body=body, crc=5) + m[0], 0, PFLUSH, parts=[PFLUSH, PFLUSH],
            multi_status=605, source=GZ_A + ":72-73")
    # BGZF: the 'BC' sub-field beside others; the engine decodes such files in one launch and falls back to the walk on any doubt
    bg = [F.bgzf_member(PA, before=[("X", "Y", b"12")], behind=[("Z", "Z", b"")]), F.bgzf_member(PB), F.bgzf_member(P0)]
    add("bgzf-three-members-bc-beside-other-fields", bg[0] + bg[1] + bg[2], 0, PA, parts=[PA, PB, P0], source=GZ_H + ":125-155")
    add("bgzf-bc-of-length-3", F.bgzf_member(PA, bc_len=3) + bg[1], 0, PA, parts=[PA, PB], source=GZ_H + ":125-155")
    add("bgzf-bsize-one-short", F.bgzf_member(PA, bsize=len(F.bgzf_member(PA)) - 2) + bg[1], 0, PA, parts=[PA, PB], source=GZ_A + ":67-76 (BSIZE is no field of the reference's)")
    add("bgzf-bsize-into-the-next-member", F.bgzf_member(PA, bsize=len(F.bgzf_member(PA)) + 20) + bg[1] + bg[2], 0, PA, parts=[PA, PB, P0], source=GZ_A + ":67-76")
    add("bgzf-member-2-wrong-crc", bg[0] + F.bgzf_member(PB, crc=3) + bg[2], 0, PA, parts=[PA, PB], multi_status=605, source=GZ_A + ":72-73")
    add("bgzf-member-2-wrong-isize", bg[0] + F.bgzf_member(PB, isize=3) + bg[2], 0, PA, parts=[], multi_status=606, source=GZ_A + ":95")
    add("bgzf-then-a-plain-member", bg[0] + bg[1] + m[2], 0, PA, parts=[PA, PB, PC], source=GZ_A + ":67-76")
    return cases


# ------------------------------------------------------------------------------------------------------------------------------ zlib
@functools.lru_cache(maxsize=None)
def zlib_cases():
    cases = []
    Z = F.zlib_stream
    def add(name, data, status, out=b"", **kw):
        _case(cases, "zlib", name, data, status, out, **kw)
    for p in (P0, P1, P100, P5000):
        add("valid-%d" % len(p), Z(p), 0, p, source=ZL_A + ":41")
    for lv in range(4):
        add("valid-flevel-%d" % lv, Z(P100, flevel=lv), 0, P100, source=ZL_H + ":79 (every value is a level)")
    for ci in range(8):
        add("valid-cinfo-%d" % ci, Z(P100, cinfo=ci), 0, P100, source=ZL_H + ":63")
    add("empty-input", b"", 701, stage="header", source=ZL_H + ":49")
    add("one-byte", b"\x78", 701, stage="header", source=ZL_H + ":49")
    add("cm-7", Z(P100, cm=7), 701, stage="header", source=ZL_H + ":57")
    add("cm-15", Z(P100, cm=15), 701, stage="header", source=ZL_H + ":57")
    add("cinfo-8", Z(P100, cinfo=8), 702, stage="header", source=ZL_H + ":63")
    add("cinfo-15", Z(P100, cinfo=15), 702, stage="header", source=ZL_H + ":63")
    right = Z(P100)[1] & 31
    add("fcheck-one-more", Z(P100, fcheck=right + 1), 703, stage="header", source=ZL_H + ":83")
    add("fcheck-one-less", Z(P100, fcheck=right - 1), 703, stage="header", source=ZL_H + ":83")
    add("cm-and-fcheck-wrong", Z(P100, cm=7, fcheck=(Z(P100, cm=7)[1] & 31) ^ 1), 701, stage="header", source=ZL_H + ":57 before :83")
    add("cinfo-and-fcheck-wrong", Z(P100, cinfo=8, fcheck=(Z(P100, cinfo=8)[1] & 31) ^ 1), 702, stage="header", source=ZL_H + ":63 before :83")
    add("cm-and-cinfo-wrong", Z(P100, cm=7, cinfo=8), 701, stage="header", source=ZL_H + ":57 before :63")
    add("fdict-with-4-bytes", Z(P100, fdict=True, dictid=b"\x01\x02\x03\x04"), 0, P100, source=ZL_H + ":87-90")
    add("fdict-with-3-bytes", Z(P0, fdict=True, dictid=b"\x01\x02\x03", body=b"", trailer=b""), 703, stage="header", source=ZL_H + ":88")
    add("fdict-with-0-bytes", Z(P0, fdict=True, dictid=b"", body=b"", trailer=b""), 703, stage="header", source=ZL_H + ":88")
    add("fdict-with-4-bytes-and-nothing-else", Z(P0, fdict=True, body=b"", trailer=b""), 102, source=DEFL + ":37")
    add("fdict-and-fcheck-wrong", Z(P0, fdict=True, dictid=b"", body=b"", trailer=b"", fcheck=(Z(P0, fdict=True)[1] & 31) ^ 1), 703, stage="header",
        source=ZL_H + ":83")
    add("header-alone", Z(P0, body=b"", trailer=b""), 102, source=DEFL + ":37")
    add("adler-wrong", Z(P100, adler=1), 705, P100, stage="trailer", source=ZL_A + ":38")
    add("adler-little-endian", Z(P100, trailer=struct.pack("<I", F.adler32(P100))), 705, P100, stage="trailer", source=ZL_A + ":37 (byteSwapped)")
    for k in range(4):
        add("trailer-of-%d-bytes" % k, Z(P100, trailer=struct.pack(">I", F.adler32(P100))[:k]), 705, P100, stage="trailer", source=ZL_A + ":34")
    add("deflate-error-and-wrong-adler", Z(P0, body=BAD_TYPE, adler=5), 102, source=DEFL + ":239")
    add("deflate-error-and-no-trailer", Z(b"abcde", body=BAD_STORED, trailer=b""), 101, source=DEFL + ":57")
    add("garbage-behind-the-trailer", Z(P100) + b"\xAA" * 7, 0, P100, source=ZL_A + ":41")
    mid = bytes(range(65, 91))
    add("body-ends-in-mid-byte", Z(mid, body=F.deflate_mid_byte(mid)), 0, mid, source=ZL_A + ":32")
    add("body-ends-in-mid-byte-adler-wrong", Z(mid, body=F.deflate_mid_byte(mid), adler=9), 705, mid, stage="trailer", source=ZL_A + ":32,38")
    for tag, full in (("full-flush", True), ("sync-flush", False)):
        body = F.deflate_flushed(PFLUSH, full=full)
        add("flushed-%s" % tag, Z(PFLUSH, body=body), 0, PFLUSH, source=ZL_A + ":41")
        add("flushed-%s-adler-wrong" % tag, Z(PFLUSH, body=body, adler=77), 705, PFLUSH, stage="trailer", source=ZL_A + ":38")
        add("flushed-%s-no-trailer" % tag, Z(PFLUSH, body=body, trailer=b""), 705, PFLUSH, stage="trailer", source=ZL_A + ":34")
    return cases


# ------------------------------------------------------------------------------------------------------------------------------- LZ4
DICT = bytes(range(48, 112))               # 64 bytes, all different
OFFSET_0 = L4.block([(b"abcd", 0, 4)], b"12345")          # DataError.corrupted (LZ4.swift:382)
LITERALS_PAST_END = bytes([0x50]) + b"ab"                 # five literals announced, two there: DataError.truncated (LZ4.swift:364)


@functools.lru_cache(maxsize=None)
def lz4_cases():
    cases = []
    Fr, lit = F.lz4_frame, F.lz4_literals
    def add(name, data, status, out=b"", **kw):
        _case(cases, "lz4", name, data, status, out, **kw)
    def comp(p):
        return (corpus.lz4_block(p), False)
    add("valid-no-blocks", Fr([]), 0, b"", source=LZ + ":191,284")
    add("valid-1-literal", Fr([(lit(P1), False)]), 0, P1, source=LZ + ":329")
    add("valid-100-stored", Fr([(P100, True)]), 0, P100, source=LZ + ":316")
    add("valid-5000", Fr([comp(P5000)]), 0, P5000, source=LZ + ":305")
    two = [comp(P70001[:65536]), comp(P70001[65536:])]
    add("valid-70001-two-blocks", Fr(two, bd=0x40), 0, P70001, source=LZ + ":305")
    add("valid-70001-two-dependent-blocks", Fr(two, bd=0x40, independent=False), 0, P70001, source=LZ + ":311")
    add("valid-every-field", Fr([comp(P5000), (P100, True)], block_checksum=True, content_size=5100, content_checksum=F.xxh32(P5000 + P100)), 0, P5000 + P100,
        source=LZ + ":300,320,326")
    add("valid-empty-stored-block-is-no-end-mark", Fr([(b"", True), (P100, True)]), 0, P100, source=LZ + ":284-289")
    # decompress(data:) itself
    add("three-bytes", b"\x04\x22\x4d", 501, stage="header", source=LZ + ":75", multi_status=501)
    add("empty-input", b"", 501, stage="header", source=LZ + ":75; :123")
    add("unknown-magic", Fr([], magic=0x184D2205), 502, stage="header", source=LZ + ":89; :137")
    # process(frame:): the descriptor
    add("6-bytes-behind-the-magic", Fr([], cut=10), 501, stage="header", source=LZ + ":191")
    for v in (0, 2, 3):
        add("version-%d" % v, Fr([(P100, True)], version=v), 502, stage="header", source=LZ + ":198")
    add("reserved-flg-bit", Fr([(P100, True)], reserved=1), 502, stage="header", source=LZ + ":198")
    for bd in range(0x00, 0x100, 0x10):
        if bd in (0x40, 0x50, 0x60, 0x70):
            add("bd-%02x" % bd, Fr([(P100, True)], bd=bd), 0, P100, source=LZ + ":216-224")
        else:
            add("bd-%02x" % bd, Fr([(P100, True)], bd=bd), 502, stage="header", source=LZ + ":227")
    for bd in (0x41, 0x48, 0x7F):
        add("bd-%02x-low-bits" % bd, Fr([(P100, True)], bd=bd), 502, stage="header", source=LZ + ":227")
    add("version-and-bd-wrong-and-too-short", Fr([], version=0, bd=0, cut=10), 501, stage="header", source=LZ + ":191 before :198")
    add("content-size-13-bytes-left", Fr([], content_size=0), 0, b"", source=LZ + ":234")
    add("content-size-12-bytes-left", Fr([], content_size=0, cut=-1), 501, stage="header", source=LZ + ":234")
    add("content-size-2^63", Fr([(P100, True)], content_size=1 << 63), 504, stage="header", source=LZ + ":240")
    add("content-size-2^63-1", Fr([(P100, True)], content_size=(1 << 63) - 1), 502, stage="trailer", source=LZ + ":240 passes; :320")
    add("content-size-2^63-and-header-checksum-wrong", Fr([], content_size=1 << 63, header_checksum=0), 504, stage="header", source=LZ + ":240 before :274")
    add("dict-id-without-a-dictionary", Fr([(P100, True)], dict_id=5), 502, stage="header", source=LZ + ":250")
    add("dict-id-without-a-dictionary-8-bytes-left", Fr([], dict_id=5, cut=-1), 502, stage="header", source=LZ + ":250 before :254")
    add("dict-id-9-bytes-left", Fr([], dict_id=5), 0, b"", dictionary=DICT, source=LZ + ":254")
    add("dict-id-8-bytes-left", Fr([], dict_id=5, cut=-1), 501, dictionary=DICT, stage="header", source=LZ + ":254")
    add("dict-id-with-an-empty-dictionary", Fr([(P100, True)], dict_id=5), 0, P100, dictionary=b"", source=LZ + ":250 (not nil)")
    add("dict-id-2^31", Fr([(P100, True)], dict_id=1 << 31), 0, P100, dictionary=DICT, source=LZ + ":259 (Int is 64 bits)")
    add("dict-id-2^32-1-given-too", Fr([(P100, True)], dict_id=0xFFFFFFFF), 0, P100, dictionary=DICT, dict_id=0xFFFFFFFF, source=LZ + ":259,268")
    add("dict-ids-equal", Fr([(P100, True)], dict_id=5), 0, P100, dictionary=DICT, dict_id=5, source=LZ + ":268")
    add("dict-ids-differ", Fr([(P100, True)], dict_id=5), 502, dictionary=DICT, dict_id=6, stage="header", source=LZ + ":268")
    add("dict-ids-differ-2^31", Fr([(P100, True)], dict_id=1 << 31), 502, dictionary=DICT, dict_id=0, stage="header", source=LZ + ":268")
    add("dict-id-given-but-none-stored", Fr([(P100, True)]), 0, P100, dictionary=DICT, dict_id=6, source=LZ + ":266")
    add("header-checksum-wrong", Fr([(P100, True)], header_checksum=(F.xxh32(bytes([0x60, 0x70])) >> 8 & 0xFF) ^ 1), 502, stage="header", source=LZ + ":274")
    full = struct.pack("<BBQI", 0x69, 0x70, 100, 5)
    add("header-checksum-right-over-all-fields", Fr([(P100, True)], content_size=100, dict_id=5), 0, P100, dictionary=DICT, source=LZ + ":272-274")
    add("header-checksum-wrong-over-all-fields", Fr([(P100, True)], content_size=100, dict_id=5, header_checksum=(F.xxh32(full) >> 8 & 0xFF) ^ 0x80), 502,
        dictionary=DICT, stage="header", source=LZ + ":274")
    add("header-checksum-of-flg-and-bd-alone", Fr([(P100, True)], content_size=100, dict_id=5, header_checksum=F.xxh32(full[:2]) >> 8 & 0xFF), 502,
        dictionary=DICT, stage="header", source=LZ + ":272 (the optional fields are hashed)")
    add("header-checksum-without-the-dict-id", Fr([(P100, True)], content_size=100, dict_id=5, header_checksum=F.xxh32(full[:10]) >> 8 & 0xFF), 502,
        dictionary=DICT, stage="header", source=LZ + ":272")
    assert F.xxh32(full[:2]) >> 8 & 0xFF != F.xxh32(full) >> 8 & 0xFF != F.xxh32(full[:10]) >> 8 & 0xFF
    # the blocks
    big = corpus.p_rand(65537, 9)
    add("block-of-max-bytes", Fr([(big[:65536], True)], bd=0x40), 0, big[:65536], source=LZ + ":292")
    add("block-of-max-plus-1-bytes", Fr([(big, True)], bd=0x40), 502, stage="header", source=LZ + ":292")
    add("compressed-block-of-max-plus-1-bytes", Fr([(lit(big[:65000]) + bytes(65537 - len(lit(big[:65000]))), False)], bd=0x40), 502, stage="header", source=LZ + ":292")
    add("no-end-mark-behind-a-block", Fr([(P100, True)], end_mark=False), 501, stage="header", source=LZ + ":295")
    add("block-with-size-plus-3-left", Fr([(P100, True)], cut=-1), 501, stage="header", source=LZ + ":295")
    add("block-with-size-plus-8-left", Fr([(P100, True)], block_checksum=True), 0, P100, source=LZ + ":295")
    add("block-with-size-plus-7-left", Fr([(P100, True)], block_checksum=True, cut=-1), 501, stage="header", source=LZ + ":295")
    add("no-end-mark-behind-a-decoded-block", Fr([comp(P5000), (P100, True)], end_mark=False), 501, source=LZ + ":295")
    add("end-mark-cut", Fr([(P100, True)], cut=-2) + b"", 501, stage="header", source=LZ + ":295")
    add("no-end-mark-at-all", Fr([], end_mark=False), 501, stage="header", source=LZ + ":191")
    add("block-checksum-wrong-stored", Fr([(P100, True, None, F.xxh32(P100) ^ 1)], block_checksum=True), 502, stage="header", source=LZ + ":300")
    c5000 = corpus.lz4_block(P5000)
    add("block-checksum-wrong-compressed", Fr([(c5000, False, None, F.xxh32(c5000) ^ 1)], block_checksum=True), 502, stage="header", source=LZ + ":300")
    add("block-checksum-of-the-output-not-the-block", Fr([(c5000, False, None, F.xxh32(P5000))], block_checksum=True), 502, stage="header", source=LZ + ":300")
    add("content-size-one-more", Fr([comp(P5000)], content_size=5001), 502, stage="trailer", source=LZ + ":320")
    add("content-size-one-less", Fr([comp(P5000)], content_size=4999), 502, stage="trailer", source=LZ + ":320")
    add("content-size-and-checksum-wrong", Fr([comp(P5000)], content_size=4999, content_checksum=1), 502, stage="trailer", source=LZ + ":320 before :326")
    add("content-checksum-wrong", Fr([comp(P5000)], content_checksum=F.xxh32(P5000) ^ 1), 503, P5000, parts=[P5000], stage="trailer", source=LZ + ":326")
    add("content-checksum-cut", Fr([comp(P5000)], content_checksum=struct.pack("<I", F.xxh32(P5000))[:3]), 501, stage="trailer", source=LZ + ":324")
    add("content-checksum-absent", Fr([comp(P5000)], content_checksum=b""), 501, stage="trailer", source=LZ + ":324")
    # precedence inside one block (:292-301)
    add("max-plus-1-and-wrong-checksum", Fr([(big, True, None, 1)], bd=0x40, block_checksum=True), 502, stage="header", source=LZ + ":292 before :300")
    add("max-plus-1-and-truncated", Fr([(big[:100], True, 65537 | 0x80000000)], bd=0x40), 502, stage="header", source=LZ + ":292 before :295")
    add("wrong-checksum-and-less-than-size-plus-8", Fr([(P100, True, None, 1)], block_checksum=True, cut=-1), 501, stage="header", source=LZ + ":295 before :300")
    # the order that discovery-first can break: the reference decodes block k before it looks at block k + 1
    for tag, ind in (("independent", True), ("dependent", False)):
        add("%s-offset-0-then-no-end-mark" % tag, Fr([(OFFSET_0, False)], independent=ind, end_mark=False), 501, stage="header", source=LZ + ":295 (the guard wants the end mark's four bytes)")
        add("%s-offset-0-then-end-mark-cut-behind-a-second-block" % tag, Fr([(OFFSET_0, False), (P100, True)], independent=ind, end_mark=False), 502, source=LZ + ":382 before :295")
        add("%s-good-then-offset-0-then-cut" % tag, Fr([comp(P5000), (OFFSET_0, False), (P100, True)], independent=ind, end_mark=False), 502, source=LZ + ":382 before :295")
        add("%s-good-then-cut" % tag, Fr([comp(P5000), (P100, True)], independent=ind, end_mark=False), 501, source=LZ + ":295")
        add("%s-literals-past-end-then-max-plus-1" % tag, Fr([(LITERALS_PAST_END, False), (big, True)], independent=ind, bd=0x40), 501, source=LZ + ":364 before :292")
        add("%s-max-plus-1-then-literals-past-end" % tag, Fr([(big, True), (LITERALS_PAST_END, False)], independent=ind, bd=0x40), 502, stage="header", source=LZ + ":292")
        add("%s-wrong-block-checksum-then-undecodable" % tag, Fr([(P100, True, None, 1), (LITERALS_PAST_END, False)], independent=ind, block_checksum=True), 502,
            stage="header", source=LZ + ":300")
        add("%s-undecodable-then-wrong-block-checksum" % tag, Fr([(LITERALS_PAST_END, False), (P100, True, None, 1)], independent=ind, block_checksum=True), 501,
            source=LZ + ":364 before :300")
        add("%s-offset-0-then-wrong-content-size-and-checksum" % tag, Fr([(OFFSET_0, False)], independent=ind, content_size=3, content_checksum=1), 502, source=LZ + ":382")
    # dependent blocks and `out.isEmpty` (:307): while the frame has produced nothing, the window is the dictionary
    back16 = L4.block([(b"", 16, 8)], b"ZZZZZ")
    back17 = L4.block([(b"", 17, 8)], b"ZZZZZ")
    S16 = b"ABCDEFGHIJKLMNOP"
    for tag, first in (("empty-stored", (b"", True)), ("empty-compressed", (b"\x00", False))):
        add("dependent-%s-first-block-dictionary-used-again" % tag, Fr([first, (back16, False)], independent=False), 0, DICT[48:56] + b"ZZZZZ", dictionary=DICT, source=LZ + ":307-309")
        add("dependent-%s-first-block-no-dictionary" % tag, Fr([first, (back16, False)], independent=False), 502, source=LZ + ":311,382")
        add("dependent-%s-first-block-reaches-past-the-dictionary" % tag, Fr([first, (L4.block([(b"", 65, 8)], b"ZZZZZ"), False)], independent=False), 502, dictionary=DICT,
            source=LZ + ":382")
    add("dependent-stored-first-block-output-used", Fr([(S16, True), (back16, False)], independent=False), 0, S16 + S16[:8] + b"ZZZZZ", dictionary=DICT, source=LZ + ":311")
    add("dependent-stored-first-block-dictionary-out-of-reach", Fr([(S16, True), (back17, False)], independent=False), 502, dictionary=DICT, source=LZ + ":311,382")
    add("dependent-stored-first-block-no-dictionary", Fr([(S16, True), (back16, False)], independent=False), 0, S16 + S16[:8] + b"ZZZZZ", source=LZ + ":311")
    add("dependent-first-block-reaches-into-the-dictionary", Fr([(back16, False), (back17, False)], independent=False), 502, dictionary=DICT, source=LZ + ":311,382 (13 bytes of output)")
    add("independent-every-block-sees-the-dictionary", Fr([(S16, True), (back17, False)]), 0, S16 + DICT[47:55] + b"ZZZZZ", dictionary=DICT, source=LZ + ":305")
    # legacy frames, skippable frames, several frames
    lg = F.lz4_legacy([lit(PA), corpus.lz4_block(P5000)])
    add("legacy-two-blocks", lg, 0, PA + P5000, source=LZ + ":160-186")
    add("legacy-no-blocks", F.lz4_legacy([]), 0, b"", source=LZ + ":164")
    add("legacy-then-a-frame", lg + Fr([(PB, True)]), 0, PA + P5000, parts=[PA + P5000, PB], source=LZ + ":168-171")
    add("legacy-then-a-legacy-frame", lg + F.lz4_legacy([lit(PB)]), 0, PA + P5000, parts=[PA + P5000, PB], source=LZ + ":168-171")
    for nib in (0, 15):
        add("legacy-then-skippable-%x" % nib, lg + F.lz4_skippable(b"skip", nib), 0, PA + P5000, parts=[PA + P5000], source=LZ + ":168-171")
    add("legacy-then-almost-a-magic", F.lz4_legacy([lit(PA)]) + struct.pack("<I", 0x184D2A60), 501, source=LZ + ":177")
    add("legacy-block-longer-than-the-rest", F.lz4_legacy([(lit(PA), len(lit(PA)) + 1)]), 501, stage="header", source=LZ + ":177")
    add("legacy-3-bytes-behind-a-block", lg + b"\x01\x02\x03", 501, source=LZ + ":165")
    add("legacy-undecodable-block-then-3-bytes", F.lz4_legacy([OFFSET_0]) + b"\x01\x02\x03", 502, source=LZ + ":382 before :165")
    for nib in range(16):
        add("skippable-%x-then-a-frame" % nib, F.lz4_skippable(b"xyz", nib) + Fr([(PA, True)]), 0, PA, source=LZ + ":83-85; :132-133")
    add("skippable-larger-than-the-rest", F.lz4_skippable(b"xyz", size=4) + b"", 501, stage="header", source=LZ + ":152")
    add("skippable-size-cut", F.lz4_skippable(b"")[:7], 501, stage="header", source=LZ + ":149")
    add("skippable-alone", F.lz4_skippable(b"xyz"), 501, parts=[], multi_status=0, stage="header", source=LZ + ":85,75; multiDecompress: :143")
    add("skippable-of-size-0-then-a-frame", F.lz4_skippable(b"") + Fr([(PA, True)]), 0, PA, source=LZ + ":152-154")
    add("skippable-drops-the-dictionary", F.lz4_skippable(b"xyz") + Fr([(PA, True)], dict_id=5), 502, parts=[PA], multi_status=0, dictionary=DICT, stage="header",
        source=LZ + ":85 (decompress(data:) again, no dictionary); :131")
    add("magic-5f-plus-1", struct.pack("<II", 0x184D2A60, 0), 502, stage="header", source=LZ + ":89")
    f1, f2, f3 = Fr([comp(P5000)], content_checksum=F.xxh32(P5000)), Fr([(PB, True)], content_checksum=F.xxh32(PB)), Fr([(PC, True)])
    add("three-frames", f1 + f2 + f3, 0, P5000, parts=[P5000, PB, PC], source=LZ + ":120-143")
    add("three-frames-mismatch-in-the-second", f1 + Fr([(PB, True)], content_checksum=1) + f3, 0, P5000, parts=[PB], multi_status=503, source=LZ + ":327 ([out] of that frame alone)")
    add("three-frames-header-error-in-the-third", f1 + f2 + Fr([(PC, True)], bd=0x30), 0, P5000, parts=[], multi_status=502, source=LZ + ":227")
    add("two-frames-then-3-bytes", f1 + f2 + b"\x04\x22\x4d", 0, P5000, parts=[], multi_status=501, source=LZ + ":123")
    add("two-dependent-frames-and-a-skippable", Fr(two, bd=0x40, independent=False) + F.lz4_skippable(b"s") + Fr([(S16, True), (back16, False)], independent=False), 0, P70001,
        parts=[P70001, S16 + S16[:8] + b"ZZZZZ"], source=LZ + ":120-143")
    return cases


# -------------------------------------------------------------------------------------------------------------------------------- xz
def delta_decode(data, distance=1):
    """DeltaFilter.decode (DeltaFilter.swift:11-33) in its plain form: out[i] = in[i] + out[i - distance]."""
    out = bytearray(len(data))
    for i, b in enumerate(data):
        out[i] = (b + (out[i - distance] if i >= distance else 0)) & 0xFF
    return bytes(out)


def _runs_block(parts):
    """A block whose LZMA2 data resets the dictionary in front of every part: what "lzma2_run_bytes" cuts into units."""
    import _emu_lzma2_runs as R
    return X.block(b"".join(parts), comp=R.recipe(list(parts)), dict_byte=R.RECIPE_DICT_BYTE)


@functools.lru_cache(maxsize=None)
def xz_cases():
    cases = []
    S, B = X.stream, X.block
    def add(name, data, status, out=b"", **kw):
        if "stage" not in kw and status not in (0, 807) and re.match(re.escape(XA) + r":(1[3-9]\d|2\d\d)", kw["source"]):
            kw["stage"] = "trailer"                        # processIndex, processFooter, processPadding: behind every decode of the stream
        _case(cases, "xz", name, F.Built.of(data.stream, blocks=data.blocks) if isinstance(data, X.Built) else data, status, out, **kw)
    checks = {"none": X.CHECK_NONE, "crc32": X.CHECK_CRC32, "crc64": X.CHECK_CRC64, "sha256": X.CHECK_SHA256}
    add("valid-no-blocks-32-bytes", S([]), 0, b"", source=XA + ":100-101")
    for tag, ck in checks.items():
        add("valid-%s" % tag, S([B(P100)], check=ck), 0, P100, source=XA + ":106-121")
        add("valid-two-blocks-%s" % tag, S([B(P5000), B(P1)], check=ck), 0, P5000 + P1, source=XA + ":98-124")
    add("valid-empty-block", S([B(P0)]), 0, b"", source=XA + ":104")
    add("valid-sizes-absent", S([B(P100, comp_size=None, uncomp_size=None)]), 0, P100, source=XB + ":32-35")
    add("valid-70001-in-two-blocks", S([B(P70001[:65536]), B(P70001[65536:])], check=X.CHECK_CRC64), 0, P70001, source=XA + ":98-124")
    # the archive and the stream header
    add("31-bytes", S([]).stream[:31], 801, stage="header", source=XA + ":39")
    add("empty-input", b"", 0, b"", parts=[], stage="header", source=XA + ":37 (no stream at all)")
    add("magic-wrong", S([B(P100)], magic=b"\xFD7zXZ\x01"), 801, stage="header", source=XS + ":35")
    add("header-crc-wrong", S([B(P100)], header_crc=1), 803, stage="header", source=XS + ":43")
    for bit in range(8):
        add("stream-flags-first-byte-bit-%d" % bit, S([B(P100)], flags=bytes([1 << bit, 1])), 802, stage="header", source=XS + ":48")
    for bit in range(4, 8):
        add("stream-flags-second-byte-bit-%d" % bit, S([B(P100)], flags=bytes([0, 1 | 1 << bit])), 802, stage="header", source=XS + ":48")
    for t in (2, 3, 5, 9, 11, 15):
        add("check-type-%d-unassigned" % t, S([B(P100)], check=t), 802, stage="header", source=XS + ":52-55")
    add("reserved-flags-and-wrong-header-crc", S([B(P100)], flags=b"\x01\x01", header_crc=1), 803, stage="header", source=XS + ":43 before :48")
    # the block header
    for bit in (0x04, 0x08, 0x10, 0x20):
        add("block-flags-reserved-%02x" % bit, S([B(P100, flags=0xC0 | bit)]), 802, stage="header", source=XB + ":28")
    add("block-flags-reserved-and-header-crc-wrong", S([B(P100, flags=0xC4, header_crc=1)]), 802, stage="header", source=XB + ":28 before :73")
    n = len(X.raw_lzma2(P100))
    add("compressed-size-one-more", S([B(P100, comp_size=n + 1)]), 806, source=XB + ":80")
    add("compressed-size-one-less", S([B(P100, comp_size=n - 1)]), 806, source=XB + ":80")
    add("uncompressed-size-one-more", S([B(P100, uncomp_size=101)]), 806, source=XB + ":81")
    add("uncompressed-size-one-less", S([B(P100, uncomp_size=99)]), 806, source=XB + ":81")
    add("compressed-size-absent-uncompressed-wrong", S([B(P100, comp_size=None, uncomp_size=99)]), 806, source=XB + ":81")
    add("both-sizes-wrong-and-check-wrong", S([B(P100, comp_size=n + 1, uncomp_size=99, check_field=b"\0\0\0\0")]), 806, source=XB + ":80 before " + XA + ":111")
    add("integer-of-9-bytes", S([B(P100, uncomp_size=1 << 56)]), 806, source=MB + ":19 passes (i = 8 at the ninth byte); " + XB + ":81")
    add("integer-of-10-bytes", S([B(P100, uncomp_size=b"\x80" * 9 + b"\x01")]), 809, stage="header", source=MB + ":19 (i >= 9)")
    add("integer-ending-in-00", S([B(P100, uncomp_size=b"\xE4\x00")]), 809, stage="header", source=MB + ":19 (byte == 0x00)")
    add("compressed-size-integer-ending-in-00", S([B(P100, comp_size=b"\x80\x80\x00")]), 809, stage="header", source=MB + ":19")
    add("filter-id-2^62", S([B(P100, filters=[(1 << 62, b"")])]), 804, stage="header", source=XB + ":40")
    add("filter-id-2^62-minus-1", S([B(P100, filters=[((1 << 62) - 1, b"")])]), 804, stage="header", source=XB + ":60")
    add("filter-id-integer-of-10-bytes", S([B(P100, filters=[(b"\x80" * 9 + b"\x01", b"")])]), 809, stage="header", source=MB + ":19")
    add("lzma2-property-size-2", S([B(P100, filters=[(0x21, bytes([X.DICT_BYTE, 0]), 2)])]), 401, stage="header", source=XB + ":47")
    add("lzma2-property-size-0", S([B(P100, filters=[(0x21, b"", 0)])]), 401, stage="header", source=XB + ":47")
    for db in (40, 41, 0x40, 0x80 | X.DICT_BYTE):
        add("lzma2-dictionary-byte-%02x" % db, S([B(P100, dict_byte=db)]), 401, source="LZMA2Decoder.swift:21-25")
    add("unknown-filter-x86", S([B(P100, filters=[(0x04, b""), (0x21, bytes([X.DICT_BYTE]))])]), 804, stage="header", source=XB + ":60")
    add("lzma1-filter", S([B(P100, filters=[(0x4000000000000001, b"")])]), 804, stage="header", source=XB + ":40")
    dq = bytes((i * 7 + 3) & 0xFF for i in range(300))
    d1, d3 = delta_decode(dq), delta_decode(delta_decode(delta_decode(dq, 1), 2), 256)
    add("delta-then-lzma2", S([B(d1, comp=X.raw_lzma2(dq), filters=[(0x03, b"\x00"), (0x21, bytes([X.DICT_BYTE]))])]), 0, d1, source=XB + ":52-58,78")
    add("four-filters", S([B(d3, comp=X.raw_lzma2(dq), filters=[(0x03, b"\xFF"), (0x03, b"\x01"), (0x03, b"\x00"), (0x21, bytes([X.DICT_BYTE]))])]), 0, d3,
        source=XB + ":27,38,78 (the last filter reads the archive)")
    add("delta-property-size-2", S([B(P100, filters=[(0x03, b"\x00\x00", 2), (0x21, bytes([X.DICT_BYTE]))])]), 802, stage="header", source=XB + ":55")
    add("filter-count-says-2-but-one-is-there", S([B(P100, flags=0x01, comp_size=None, uncomp_size=None)]), 804, stage="header", source=XB + ":38-60 (the padding's 0x00 is read as a filter id)")
    bare = dict(comp_size=None, uncomp_size=None)          # flags, id, property size, property: a header of 5 bytes and 3 of padding
    add("header-padding-longer", S([B(P100, header_padding=bytes(7), **bare)]), 0, P100, source=XB + ":65-69")
    add("header-padding-non-zero", S([B(P100, header_padding=b"\x00\x00\x01", **bare)]), 808, stage="header", source=XB + ":67")
    add("header-padding-non-zero-and-crc-wrong", S([B(P100, header_padding=b"\x01\x00\x00", header_crc=1, **bare)]), 808, stage="header", source=XB + ":67 before :73")
    add("block-header-crc-wrong", S([B(P100, header_crc=1)]), 803, stage="header", source=XB + ":73")
    longer = S([B(P100, size_byte=3, **bare)])
    assert longer.stream[20] != 0                          # the first byte of the header's CRC, now read as padding
    add("header-size-byte-one-more", longer, 808, stage="header", source=XB + ":65-68 (the stored CRC is read as padding)")
    # block padding and the check field
    def two_of_padding(p):
        r = S([B(p)]).blocks[0]
        return (r["data"] - r["header"] + r["comp"]) % 4 == 2 and zlib.crc32(p) & 0xFF != 0
    pay = next(p for p in (corpus.p_text(100 + k, 20 + k) for k in range(32)) if two_of_padding(p))
    add("block-padding-non-zero", S([B(pay, block_padding=b"\x00\x01")]), 808, source=XB + ":90")
    add("block-padding-one-short", S([B(pay, block_padding=b"\x00")]), 808, source=XB + ":90 (the first byte of the check is read as padding)")
    add("block-padding-one-more", S([B(pay, block_padding=b"\x00\x00\x00")]), 807, pay, parts=[pay], source=XA + ":110-112 (the check is read one byte early)")
    for tag, ck in checks.items():
        if ck:
            field = bytearray(X.check_field(ck, P100))
            field[-1] ^= 0x80
            add("check-wrong-%s" % tag, S([B(P100, check_field=bytes(field))], check=ck), 807, P100, parts=[P100], source=XA + ":109-120,44-45")
            add("check-wrong-%s-in-block-2-of-3" % tag, S([B(PA), B(PB, check_field=bytes(field)), B(PC)], check=ck), 807, PA + PB, parts=[PA + PB], source=XA + ":105,109-120")
    # the index
    two = [B(PA), B(PB)]
    real = [(r["data"] - r["header"] + r["comp"] + r["check_size"], r["uncomp"]) for r in S(two).blocks]
    assert S(two, records=real).stream == S(two).stream
    add("record-count-one-more", S(two, count=3), 802, source=XA + ":136")
    add("record-count-one-less", S(two, count=1), 802, source=XA + ":136")
    add("record-count-integer-ending-in-00", S(two, count=b"\x82\x00"), 809, source=MB + ":19")
    for k, tag in ((0, "first"), (1, "second")):
        for d in (1, -1):
            recs = list(real)
            recs[k] = (real[k][0] + d, real[k][1])
            add("unpadded-size-of-the-%s-record-%+d" % (tag, d), S(two, records=recs), 802, source=XA + ":141")
            recs[k] = (real[k][0], real[k][1] + d)
            add("uncompressed-size-of-the-%s-record-%+d" % (tag, d), S(two, records=recs), 806, source=XA + ":145")
    add("both-sizes-of-a-record-wrong", S(two, records=[(real[0][0] + 4, 1), real[1]]), 802, source=XA + ":141 before :145")
    ipad = -len(b"\x00\x02" + b"".join(X.multibyte(a) + X.multibyte(u) for a, u in real)) % 4
    assert ipad > 0
    add("index-padding-non-zero", S(two, index_padding=bytes(ipad - 1) + b"\x01"), 808, source=XA + ":154")
    add("index-crc-wrong", S(two, index_crc=1), 803, source=XA + ":162")
    add("index-padding-non-zero-and-crc-wrong", S(two, index_padding=b"\x01" * ipad, index_crc=1), 808, source=XA + ":154 before :162")
    # the footer
    words = len(S(two).stream) and (len(b"\x00\x02" + b"".join(X.multibyte(a) + X.multibyte(u) for a, u in real)) + ipad + 4) // 4 - 1
    add("footer-crc-wrong", S(two, footer_crc=1), 803, source=XA + ":177")
    add("backward-size-one-more", S(two, backward=words + 1), 802, source=XA + ":180")
    add("backward-size-one-less", S(two, backward=words - 1), 802, source=XA + ":180")
    add("backward-size-and-footer-crc-wrong", S(two, backward=words + 1, footer_crc=1), 803, source=XA + ":177 before :180")
    add("footer-flags-another-check", S(two, footer_flags=b"\x00\x04"), 802, source=XA + ":184")
    add("footer-flags-first-byte", S(two, footer_flags=b"\x01\x01"), 802, source=XA + ":184")
    add("footer-flags-high-nibble", S(two, footer_flags=b"\x00\x11"), 802, source=XA + ":186")
    add("footer-magic-wrong", S(two, footer_magic=b"YY"), 801, source=XA + ":190")
    add("footer-flags-and-magic-wrong", S(two, footer_flags=b"\x00\x04", footer_magic=b"YY"), 802, source=XA + ":184 before :190")
    add("check-wrong-and-every-later-field-wrong", S([B(PA), B(PB, check_field=b"\1\2\3\4")], count=5, index_crc=1, footer_crc=1, footer_magic=b"ZZ"), 807, PA + PB,
        parts=[PA + PB], source=XA + ":111-112 (the stream ends there)")
    # stream padding and further streams
    one = S([B(PA)]).stream
    for k in (1, 2, 3, 5, 6, 7):
        add("stream-padding-of-%d" % k, one + bytes(k), 808, source=XA + ":209-210")
    add("stream-padding-of-4", one + bytes(4), 0, PA, source=XA + ":209-212")
    add("stream-padding-of-8", one + bytes(8), 0, PA, source=XA + ":209-212")
    add("stream-padding-non-zero-fourth-byte", one + b"\x00\x00\x00\x01", 808, source=XA + ":201-203")
    add("stream-padding-non-zero-first-byte", one + b"\x01", 801, source=XA + ":201-205,217; :39")
    add("stream-padding-non-zero-fifth-byte", one + b"\x00\x00\x00\x00\x01", 801, source=XA + ":201-205,217; :39")
    second = S([B(PB)], check=X.CHECK_CRC64).stream
    add("two-streams", one + second, 0, PA + PB, parts=[PA, PB], source=XA + ":37-48")
    add("two-streams-padding-of-4-between", one + bytes(4) + second, 0, PA + PB, parts=[PA, PB], source=XA + ":194-217")
    add("two-streams-padding-of-2-between", one + bytes(2) + second, 808, source=XA + ":201-203")
    add("second-stream-check-wrong", one + S([B(PB, check_field=bytes(8))], check=X.CHECK_CRC64).stream, 807, PA + PB, parts=[PA, PB], source=XA + ":43-45; :80-82")
    add("second-stream-first-block-fails", one + S([B(PB, filters=[(0x21, b"", 0)])]).stream, 401, source=XB + ":47")
    add("second-stream-cut-to-31-bytes", one + second[:31], 801, source=XA + ":39")
    # a file that ends inside a field: the reference's reader is asked for a byte it does not have, a Swift runtime trap.  The first
    # block is whole, so every one of these ends behind a decode; block 2's header is 01 | 80 | C8 01 | 21 01 10 | 00 | CRC
    for tag, ck, field_cut in (("crc32", X.CHECK_CRC32, 2), ("crc64", X.CHECK_CRC64, 4), ("sha256", X.CHECK_SHA256, 16)):
        pb = next(p for p in (corpus.p_text(200, 70 + k) for k in range(32)) if len(X.raw_lzma2(p)) % 4 in (1, 2))
        whole = S([B(PA), B(pb, comp_size=None, uncomp_size=b"\xC8\x01")], check=ck)
        h, chk, end = whole.blocks[1]["header"], whole.blocks[1]["check"], len(whole.stream)
        index = chk + X.CHECK_SIZE[ck]
        assert whole.blocks[1]["data"] - h == 12 and chk - (whole.blocks[1]["data"] + whole.blocks[1]["comp"]) >= 2 and whole.stream[index] == 0
        cuts = [("check-field", chk + field_cut, XA + ":110-118")]
        if ck == X.CHECK_CRC32:
            cuts += [("block-header-size-byte", h, XA + ":99"), ("block-flags", h + 1, XB + ":22"), ("integer-first-byte", h + 2, MB + ":12"),
                     ("integer-second-byte", h + 3, MB + ":18"), ("filter-property", h + 6, XB + ":50"), ("header-padding", h + 7, XB + ":66"),
                     ("header-crc", h + 10, XB + ":71"), ("block-padding", chk - 1, XB + ":89"), ("index-indicator", index, XA + ":99"),
                     ("index-count", index + 1, MB + ":12"), ("index-records", index + 3, MB + ":18"), ("index-crc", end - 14, XA + ":160"),
                     ("footer-crc", end - 10, XA + ":171"), ("footer-backward-size", end - 6, XA + ":173"), ("footer-flags", end - 3, XA + ":174"),
                     ("footer-magic", end - 1, XA + ":190")]
        for where, at, src in cuts:
            add("file-ends-in-%s-%s" % (where, tag), whole.stream[:at], TRAP, source=src + " (a read past the end)")
    # lying indexes: the engine reads the index before the walk has validated anything
    for tag, size in (("2^40", 1 << 40), ("2^62", 1 << 62)):
        add("index-says-%s-bytes-of-output" % tag, S(two, records=[(real[0][0], size), real[1]]), 806, source=XA + ":145 (the blocks are fine: the walk reaches the index)")
        add("index-says-%s-unpadded" % tag, S(two, records=[(size, real[0][1]), real[1]]), 802, source=XA + ":141")
        add("index-says-%s-and-block-2-check-wrong" % tag, S([B(PA), B(PB, check_field=b"\1\2\3\4")], records=[(real[0][0], size), (real[1][0], size)]), 807, PA + PB,
            parts=[PA + PB], source=XA + ":111-112 (the index is never reached)")
    add("index-records-swapped", S(two, records=[real[1], real[0]]), 802, source=XA + ":141")
    add("index-more-records-than-blocks", S(two, records=real + [real[0]]), 802, source=XA + ":136")
    add("index-fewer-records-than-blocks", S(two, records=real[:1]), 802, source=XA + ":136")
    add("index-more-records-and-block-1-size-wrong", S([B(PA, uncomp_size=1), B(PB)], records=real + [real[0]]), 806, source=XB + ":81 (the index is never reached)")
    add("index-points-block-2-into-block-1", S(two, records=[(8, real[0][1]), (real[0][0] + real[1][0], real[1][1])]), 802, source=XA + ":141")
    # blocks whose LZMA2 data "lzma2_run_bytes" cuts into units
    # (each part compresses to more than the 4096 bytes the tests set the knob to, and the cuts lie at multiples of 16 bytes of output)
    parts = [corpus.p_rand(6000, 40) + corpus.p_text(2000, 41), corpus.p_rand(6000, 42) + corpus.p_text(2000, 43), corpus.p_rand(5000, 44)]
    whole = b"".join(parts)
    for tag, ck in (("crc32", X.CHECK_CRC32), ("sha256", X.CHECK_SHA256)):
        add("runs-block-%s" % tag, S([_runs_block(parts), B(PA)], check=ck), 0, whole + PA, source=XA + ":98-124")
        add("runs-block-%s-check-wrong" % tag, S([_runs_block(parts), dict(_runs_block(parts), check_field=bytes(X.CHECK_SIZE[ck])), B(PA)], check=ck), 807, whole + whole,
            parts=[whole + whole], source=XA + ":109-120")
    add("runs-block-uncompressed-size-wrong", S([dict(_runs_block(parts), uncomp_size=len(whole) - 1), B(PA)]), 806, source=XB + ":81")
    add("runs-block-index-says-2^40", S([_runs_block(parts), B(PA)], records=[(1 << 40, len(whole)), (real[0][0], len(PA))]), 802, source=XA + ":141")
    return cases


# ----------------------------------------------------------------------------------------------------------------------------- bzip2
@functools.lru_cache(maxsize=None)
def bzip2_cases():
    cases = []
    Sb = F.bzip2_stream
    def add(name, data, status, out=b"", **kw):
        _case(cases, "bzip2", name, data, status, out, **kw)
    def blocks_of(p):
        return F.bzip2_blocks(bz2.compress(p, 9))
    a, b = blocks_of(PA), blocks_of(P5000)
    assert len(a) == 1 and len(b) == 1
    randomized = [(b[0][0], (b[0][1][0] | 1 << (b[0][1][1] - 1), b[0][1][1]))]     # the first bit of a block: BZip2Error.randomizedBlock (BZip2.swift:108)
    assert Sb(a, head=b"BZh9") == bz2.compress(PA, 9)
    add("valid-no-blocks", Sb([]), 0, b"", source=BZ + ":85-88")
    add("valid-one-block", Sb(a), 0, PA, source=BZ + ":78-84")
    add("valid-two-blocks", Sb(a + b), 0, PA + P5000, source=BZ + ":83-84")
    for lv in b"12345678":
        add("valid-level-%c" % lv, Sb(a, head=b"BZh" + bytes([lv])), 0, PA, source=BZ + ":65")
    add("three-bytes", b"BZh", 201, stage="header", source=BZ + ":53")
    add("empty-input", b"", 201, parts=[], multi_status=0, stage="header", source=BZ + ":53; :43 (no stream at all)")
    add("level-0", Sb(a, head=b"BZh0"), 203, stage="header", source=BZ + ":65-66")
    add("level-colon", Sb(a, head=b"BZh:"), 203, stage="header", source=BZ + ":65-66")
    add("version-i", Sb(a, head=b"BZi9"), 202, stage="header", source=BZ + ":63")
    add("magic-wrong", Sb(a, head=b"BYh9"), 201, stage="header", source=BZ + ":60")
    add("magic-and-version-and-level-wrong", Sb(a, head=b"BYi0"), 201, stage="header", source=BZ + ":60 before :63,66")
    add("version-and-level-wrong", Sb(a, head=b"BZi0"), 202, stage="header", source=BZ + ":63 before :66")
    add("header-alone", b"BZh9", 201, stage="header", source=BZ + ":71-72")
    add("header-and-72-bits", b"BZh9" + Sb([])[4:13], 201, stage="header", source=BZ + ":71-72")
    add("level-0-and-nothing-else", b"BZh0", 203, stage="header", source=BZ + ":65-66 before :71")
    add("block-crc-wrong", Sb(a, crcs=[a[0][0] ^ 1]), 210, PA, parts=[PA], source=BZ + ":81-82")
    add("block-1-crc-wrong-block-2-undecodable", Sb(a + randomized, crcs=[a[0][0] ^ 1, None]), 210, PA, parts=[PA], source=BZ + ":81-82")
    add("block-1-undecodable-block-2-crc-wrong", Sb(randomized + a, crcs=[None, a[0][0] ^ 1]), 205, source=BZ + ":108")
    add("block-2-crc-wrong", Sb(b + a, crcs=[None, a[0][0] ^ 1]), 210, P5000 + PA, parts=[P5000 + PA], source=BZ + ":80-82")
    add("stream-crc-wrong", Sb(a + b, stream_crc=1), 210, PA + P5000, parts=[PA + P5000], source=BZ + ":86-87")
    add("stream-crc-wrong-no-blocks", Sb([], stream_crc=1), 210, b"", parts=[b""], source=BZ + ":86-87")
    add("block-crc-wrong-and-stream-crc-wrong", Sb(a + b, crcs=[None, b[0][0] ^ 1], stream_crc=1), 210, PA + P5000, parts=[PA + P5000], source=BZ + ":81-82")
    add("first-mark-is-neither", Sb(a, marks=[F.BZ_BLOCK ^ 1]), 204, stage="header", source=BZ + ":89-90")
    add("second-mark-is-neither", Sb(a + b, marks=[None, F.BZ_END ^ 1]), 204, source=BZ + ":89-90")
    add("end-mark-is-neither", Sb(a, end_mark=F.BZ_END ^ 2), 204, source=BZ + ":89-90")
    add("end-mark-is-neither-and-crc-wrong", Sb(a, end_mark=F.BZ_END ^ 2, stream_crc=1), 204, source=BZ + ":89-90")
    # 79 and 80 bits behind a block: a block whose body ends one bit behind a byte, and one that ends on a byte
    def block_ending(residue):
        for k in range(64):
            p = corpus.p_text(120 + k, 60 + k)
            bl = blocks_of(p)
            if bl[0][1][1] % 8 == residue:
                return p, bl
        raise AssertionError("no block with %d bits over" % residue)
    p79, b79 = block_ending(1)
    p80, b80 = block_ending(0)
    add("80-bits-behind-a-block", Sb(b80), 0, p80, source=BZ + ":71")
    add("79-bits-behind-a-block", Sb(b79, tail_bits=79), 201, source=BZ + ":71-72")
    add("72-bits-behind-a-block", Sb(b80, tail_bits=72), 201, source=BZ + ":71-72")
    add("no-end-behind-a-block", Sb(b80, end_mark=None), 201, source=BZ + ":71-72")
    # several streams, and bytes behind the end
    s1, s2 = Sb(a), Sb(b)
    add("two-streams", s1 + s2, 0, PA, parts=[PA, P5000], source=BZ + ":43-46")
    add("second-stream-stream-crc-wrong", s1 + Sb(b, stream_crc=1), 0, PA, parts=[P5000], multi_status=210, source=BZ + ":87 (the out of that stream alone)")
    add("second-stream-block-crc-wrong", s1 + Sb(b + a, crcs=[b[0][0] ^ 1, None]), 0, PA, parts=[P5000], multi_status=210, source=BZ + ":82")
    add("second-stream-undecodable", s1 + Sb(randomized), 0, PA, parts=[], multi_status=205, source=BZ + ":108")
    add("second-stream-level-0", s1 + Sb(b, head=b"BZh0"), 0, PA, parts=[], multi_status=203, source=BZ + ":66")
    add("first-stream-crc-wrong-then-a-stream", Sb(a, stream_crc=1) + s2, 210, PA, parts=[PA], source=BZ + ":87")
    for k in (1, 3):
        add("garbage-of-%d-behind-the-end" % k, s1 + b"\xAA" * k, 0, PA, parts=[], multi_status=201, source=BZ + ":53")
    add("garbage-of-4-behind-the-end", s1 + b"\xAA" * 4, 0, PA, parts=[], multi_status=201, source=BZ + ":60")
    add("a-block-mark-behind-the-end", s1 + Sb(b)[4:], 0, PA, parts=[], multi_status=201, source=BZ + ":60")
    return cases


KINDS = {"gzip": gzip_cases, "zlib": zlib_cases, "lz4": lz4_cases, "xz": xz_cases, "bzip2": bzip2_cases}


def all_cases():
    return [c for fn in KINDS.values() for c in fn()]


# ------------------------------------------------------------------------------------------------ the engine's calls for a case
def engine_single(c):
    """(status, bytes) of the case's single-shot call through the Python mirror: the result, or what the error carries."""
    import swcompression_amd as swc
    try:
        if c.kind == "gzip":
            return 0, swc.GzipArchive.unarchive(c.data)
        if c.kind == "zlib":
            return 0, swc.ZlibArchive.unarchive(c.data)
        if c.kind == "lz4":
            return 0, swc.LZ4.decompress(c.data, c.dictionary, c.dict_id)
        if c.kind == "xz":
            return 0, swc.XZArchive.unarchive(c.data)
        return 0, swc.BZip2.decompress(c.data)
    except swc.SWCError as e:
        assert e.case == swc.STATUS[e.status][1] and type(e).__name__ == swc.STATUS[e.status][0]
        return e.status, e.data if e.data is not None else b""


def engine_multi(c):
    """(status, parts) of the case's multi call: multiUnarchive, multiDecompress, splitUnarchive."""
    import swcompression_amd as swc
    try:
        if c.kind == "gzip":
            return 0, swc.GzipArchive.multi_unarchive(c.data)
        if c.kind == "lz4":
            return 0, swc.LZ4.multi_decompress(c.data, c.dictionary, c.dict_id)
        if c.kind == "xz":
            return 0, swc.XZArchive.split_unarchive(c.data)
        return 0, swc.BZip2.multi_decompress(c.data)
    except swc.SWCError as e:
        assert e.case == swc.STATUS[e.status][1] and type(e).__name__ == swc.STATUS[e.status][0]
        return e.status, e.data if e.data is not None else []
