"""CPU tier of the container layer (csrc/framing_deflate.cpp, framing_lz4.cpp, framing_lzma.cpp, framing_bzip2.cpp, framing_many.cpp):
the archives of tests/_frames_cases.py, built field by field, with expectations stated by hand from the reference's Swift.
  - the builders against Python's own decoders and against the corpus' encoders;
  - the oracle against the hand-written expectation (two readings of the same source, neither computed from the other);
  - the library itself WITHOUT a device: a header-stage case is answered before any launch, on any machine;
  - swc_index_blocks on every case: the layout the builder recorded, and no ref that leaves the archive;
  - the same through a stand-alone program built with the address and undefined-behaviour sanitizers (tests/_frames_san.py).
The GPU tier (tests/test_gpu_frames.py) holds the engine to the same expectations."""
import bz2
import gzip
import lzma
import zlib

import pytest

import _frames_build as F
import _frames_cases as FC
import _oracle as O
import _xz_build as X
import swcompression_amd as swc
from swcompression_amd import _lib, corpus

KINDS = list(FC.KINDS)
CPU_NEVER = (901, 902)   # the oracle's output cap and the engine's "no device": no expectation is either


def _id(c):
    return "%s/%s" % (c.kind, c.name)


def oracle_single(c):
    if c.kind == "gzip":
        return O.gzip_unarchive(c.data)
    if c.kind == "zlib":
        return O.zlib_unarchive(c.data)
    if c.kind == "lz4":
        return O.lz4(c.data, c.dictionary, -1 if c.dict_id is None else c.dict_id)[:2]
    if c.kind == "xz":
        return O.xz_unarchive(c.data)
    return O.bzip2(c.data)[:2]


def oracle_multi(c):
    if c.kind == "gzip":
        return O.gzip_multi_unarchive(c.data)
    if c.kind == "lz4":
        return O.lz4_multi(c.data, c.dictionary, -1 if c.dict_id is None else c.dict_id)
    if c.kind == "xz":
        return O.xz_split_unarchive(c.data)
    return O.bzip2_multi(c.data)


# ---------------------------------------------------------------------------------------------------------------------- the cases
def test_every_case_carries_an_expectation():
    """No case is left out of anything: each has a status from include/swc_status.h (never the oracle's cap, never 'no device'), the
    bytes that go with it, a stage and a Swift line; the error cases that carry nothing carry nothing."""
    cases = FC.all_cases()
    assert len(cases) > 450 and len({_id(c) for c in cases}) == len(cases)
    carries = {"gzip": 605, "zlib": 705, "lz4": 503, "xz": 807, "bzip2": 210}
    for c in cases:
        assert c.status in swc.STATUS or c.status == 0, _id(c)
        assert c.status not in CPU_NEVER and c.multi_status not in CPU_NEVER, _id(c)
        assert ".swift:" in c.source and c.stage in ("header", "payload", "trailer"), _id(c)
        assert len(c.data) <= 200_000, _id(c)
        if c.status not in (0, carries[c.kind]):
            assert c.out == b"", _id(c)
        if c.parts is not None and c.multi_status not in (0, carries[c.kind]):
            assert c.parts == [], _id(c)
        assert (c.parts is None) == (c.kind == "zlib"), _id(c)
    by_stage = {s: sum(c.stage == s for c in cases) for s in ("header", "payload", "trailer")}
    assert by_stage["header"] > 150 and by_stage["payload"] > 150 and by_stage["trailer"] > 30, by_stage


def _valid(kind):
    return [c for c in FC.KINDS[kind]() if c.status == 0 and c.multi_status == 0]


def test_valid_gzip_cases_decode_with_python():
    for c in _valid("gzip"):
        assert gzip.decompress(c.data) == b"".join(c.parts), c.name
        assert c.out == (c.parts[0] if c.parts else b""), c.name


def test_valid_zlib_cases_decode_with_python():
    for c in _valid("zlib"):
        if c.data[1] & 0x20:   # FDICT: the reference skips the identifier (ZlibHeader.swift:87-90); zlib wants the dictionary itself
            d = zlib.decompressobj(-15)
            assert d.decompress(c.data[6:]) == c.out and zlib.adler32(c.out) == int.from_bytes(d.unused_data[:4], "big"), c.name
            continue
        d = zlib.decompressobj()
        assert d.decompress(c.data) == c.out and d.eof, c.name


def test_valid_xz_cases_decode_with_python():
    def streams(data):
        """liblzma stream by stream (Python's lzma.decompress gives up at stream padding): the padding, whole words of zeros, is skipped here."""
        out = []
        while data:
            d = lzma.LZMADecompressor(format=lzma.FORMAT_XZ)
            out.append(d.decompress(data))
            assert d.eof
            data = d.unused_data
            while data[:4] == bytes(4):
                data = data[4:]
        return out
    n = 0
    for c in _valid("xz"):
        assert streams(c.data) == c.parts and c.out == b"".join(c.parts), c.name
        n += 1
    assert n > 20


def test_valid_bzip2_cases_decode_with_python():
    for c in _valid("bzip2"):
        assert bz2.decompress(c.data) == b"".join(c.parts), c.name
        assert c.out == (c.parts[0] if c.parts else b""), c.name


def test_defaults_are_the_corpus_encoders_bytes():
    """A valid archive built from defaults is, byte for byte, what the corpus' encoder writes wherever the two make the same choice."""
    for p in (FC.P0, FC.P100, FC.P5000):
        assert F.gzip_member(p) == corpus.gzip_member(p)
        assert F.bgzf_member(p) == corpus.gzip_member(p, bgzf=True)
        assert F.zlib_stream(p) == corpus.zlib_stream(p)
        assert F.bzip2_stream(F.bzip2_blocks(bz2.compress(p, 9))) == corpus.bzip2_stream(p)
        raw = lzma.compress(p, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": 6}])
        assert X.stream([X.block(p, comp=raw, comp_size=None, uncomp_size=None, dict_byte=22)] if p else [], check=X.CHECK_CRC64).stream == corpus.xz_stream(p)
        assert X.stream([X.block(p)], check=X.CHECK_SHA256).stream == X.build([p]).stream
    p = FC.P5000
    block = (corpus.lz4_block(p), False)
    assert F.lz4_frame([block]) == corpus.lz4_frame(p)
    assert F.lz4_frame([block], block_checksum=True, content_size=len(p), content_checksum=F.xxh32(p)) == \
        corpus.lz4_frame(p, content_checksum=True, block_checksum=True, content_size=True)
    r = corpus.p_rand(100, 3)
    assert F.lz4_frame([(r, True)], bd=0x40) == corpus.lz4f_frame(r)
    assert F.lz4_frame([(r, True)], bd=0x40, content_checksum=F.xxh32(r)) == corpus.lz4f_frame(r, content_checksum=True)
    assert F.xxh32(p) == O.xxh32(p)


def test_flushed_bodies_are_cut_where_the_knob_cuts():
    """The bodies meant for "deflate_unit_bytes" and "lzma2_run_bytes" really hold several units at the values the GPU tier sets."""
    lib = _lib.load()
    try:
        assert lib.swc_set_tuning(b"deflate_unit_bytes", 1024) == 0 and lib.swc_set_tuning(b"lzma2_run_bytes", 4096) == 0
        for full in (True, False):
            assert len(swc.index_blocks("deflate", F.deflate_flushed(FC.PFLUSH, full=full))) >= 4
        c = next(c for c in FC.xz_cases() if c.name == "runs-block-crc32")
        (off, comp, _, db), _ = swc.index_blocks("xz", c.data)
        assert len(swc.index_blocks("lzma2_runs", bytes([db]) + c.data[off:off + comp])) == 3
    finally:
        lib.swc_set_tuning(b"deflate_unit_bytes", 0)
        lib.swc_set_tuning(b"lzma2_run_bytes", 0)


# ------------------------------------------------------------------------------------------- the oracle against the expectation
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_agrees_with_the_hand_written_expectation(kind):
    """Status, carried bytes and parts of every case.  Where the two differed the Swift source decided (three spots of the oracle
    handed back earlier members or streams with an error that carries nothing: oracle/rc_gzip_zlib.c, rc_lz4.c, rc_xz.c)."""
    wrong = []
    for c in FC.KINDS[kind]():
        got = oracle_single(c)
        assert got[0] != 901, c.name
        if got != (c.status, c.out):
            wrong.append((c.name, "single", got[0], len(got[1]), c.status, len(c.out), c.source))
        if c.parts is not None:
            got = oracle_multi(c)
            assert got[0] != 901, c.name
            if got != (c.multi_status, c.parts):
                wrong.append((c.name, "multi", got[0], [len(p) for p in got[1]], c.multi_status, [len(p) for p in c.parts], c.source))
    assert not wrong, wrong


# ----------------------------------------------------------------------------------------------- the library without a device
@pytest.mark.parametrize("kind", KINDS)
def test_header_stage_cases_need_no_device(kind):
    """Every case the reference answers before it decodes any payload is answered by the library before any launch: the stated
    status from the single-shot call and from swc_unarchive_many (one call for all of them), on a machine with or without a device."""
    cases = [c for c in FC.KINDS[kind]() if c.stage == "header"]
    assert len(cases) >= 10
    for c in cases:
        assert FC.engine_single(c) == (c.status, c.out), c.name
    many = [c for c in cases if c.dictionary is None]
    got = swc.unarchive_many(kind, [c.data for c in many])
    assert [(st, data) for st, data in got] == [(c.status, c.out) for c in many], [c.name for c, g in zip(many, got) if g != (c.status, c.out)]


# ------------------------------------------------------------------------------------------------------------ swc_index_blocks
INDEX_KINDS = {"gzip": ["bgzf", "gzip_members", "deflate"], "zlib": ["deflate"], "lz4": ["lz4"], "xz": ["xz", "lzma2", "lzma2_runs"], "bzip2": ["bzip2", "bzip2_marks"]}


@pytest.mark.parametrize("kind", KINDS)
def test_index_blocks_stay_inside_every_case(kind):
    """Damaged archives included: whatever swc_index_blocks returns is a status of include/swc_status.h, and every ref it lists lies
    inside the archive (bzip2: in bits)."""
    seen = 0
    for c in FC.KINDS[kind]():
        for ik in INDEX_KINDS[kind]:
            try:
                refs = swc.index_blocks(ik, c.data, flags=True)
            except swc.SWCError as e:
                assert e.status in swc.STATUS and e.status != 902, (c.name, ik, e.status)
                continue
            limit = len(c.data) * (8 if ik.startswith("bzip2") else 1)
            for off, comp, _, _, _ in refs:
                assert off <= limit and comp <= limit - off, (c.name, ik, off, comp, limit)
            seen += len(refs)
    assert seen > 20


def test_index_blocks_give_the_layout_the_builder_recorded():
    n = 0
    for c in FC.all_cases():
        lay = getattr(c.data, "layout", None)
        if not lay or c.status != 0 or c.multi_status != 0:
            continue
        n += 1
        if c.kind == "gzip" and lay["size"] >= 20:
            want = (lay["header"], lay["body"], lay["isize"], lay["header"], 0)
            assert swc.index_blocks("gzip_members", c.data, flags=True) == [want], c.name
        elif c.kind == "lz4" and "blocks" in lay and c.dictionary is None:   # (the index takes no dictionary: a frame with a dictionary ID is none it lists)
            want = [b + (1 if lay["linked"] and k else 0,) for k, b in enumerate(lay["blocks"])]
            assert swc.index_blocks("lz4", c.data, flags=True) == want, c.name
        elif c.kind == "xz":
            want = [(b["data"], b["comp"], b["uncomp"], b["dict_byte"], 0) for b in lay["blocks"]]
            got = swc.index_blocks("xz", c.data, flags=True)
            if "filters" in c.name or "delta" in c.name:
                assert got == [], c.name            # (blocks with other filter chains are left out)
            else:
                assert got == want, c.name
        elif c.kind == "bzip2":
            assert [r[0] for r in swc.index_blocks("bzip2", c.data)] == lay["blocks"], c.name
            marks = swc.index_blocks("bzip2_marks", c.data, flags=True)
            assert [(m[0], m[4]) for m in marks] == [(b, 0) for b in lay["blocks"]] + [(lay["end"], 1)], c.name
    assert n > 60
    # BGZF: the members one behind the other, each (offset of its Deflate stream, its length, ISIZE)
    members = [F.bgzf_member(FC.PA, before=[("X", "Y", b"12")]), F.bgzf_member(FC.PB), F.bgzf_member(FC.P0)]
    want, at = [], 0
    for m in members:
        want.append((at + m.layout["header"], m.layout["body"], m.layout["isize"], 0))
        at += len(m)
    assert swc.index_blocks("bgzf", b"".join(members)) == want


# ------------------------------------------------------------------------------------------------------- under the sanitizers
@pytest.mark.skipif(swc.device_available(), reason="sanitizer builds run on the CPU machine only")
def test_container_layer_under_the_sanitizers(tmp_path):
    """The library's host code with the address and undefined-behaviour sanitizers, as a child process over every case: the statuses
    of the header-stage cases (single-shot and swc_unarchive_many) and the bounds of every swc_index_blocks kind on every case, each
    archive in a heap block of exactly its length."""
    import _frames_san as S
    exe = S.build_program(tmp_path)
    out = S.run_program(exe, tmp_path, FC.all_cases())
    assert "%d cases" % len(FC.all_cases()) in out and " 0 mismatches" in out, out[-2000:]
