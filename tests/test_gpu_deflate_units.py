"""GPU tier of the Deflate units: runs of SWC_DEFLATE_JOINED / SWC_DEFLATE_OPEN jobs through the batch API on the MI355X against
units built code by code and the oracle (_deflate_units_cases), and flushed streams through the single-shot entry points against
the oracle's status, bytes and in_consumed."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import _deflate_build as DB
import _deflate_units_cases as K
import _oracle as O
import swcompression_amd as swc
from swcompression_amd import _lib, corpus
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu
DEFAULT_UNIT_BYTES = 0     # the library ships with the cut switched off: the host tests switch it on


# ------------------------------------------------------------------------------------------------------------- batch API
@pytest.fixture(scope="module")
def runs():
    """(name, units, expected per unit) of every directed run and of the sixteen residue pairs -- the reference, computed once."""
    out = [(name, run, [K.expect(u) for u in run]) for name, run in K.directed_runs().items()]
    out += [("residue-%d" % r, run, [K.expect(u) for u in run]) for r, run in enumerate(K.residue_pairs())]
    return out


def check_batch(b, runs):
    r = b.results()
    blob = b.d_out.cpu().numpy()
    base = b.d_out.data_ptr()
    i = 0
    for name, run, exp in runs:
        at = int(b._out_off[i])
        assert int(r["out"][i]) - base == at, name + ": the head's `out` moved"
        for k, (u, (st, n, cons, aux, out)) in enumerate(zip(run, exp)):
            what = "%s unit %d" % (name, k)
            assert int(r["status"][i]) == st, what
            assert int(r["aux"][i]) == aux, what + ": aux"
            assert int(r["out"][i]) - base == at, what + ": `out` is not behind the predecessor's output"
            if n is not None:
                assert (int(r["out_len"][i]), int(r["in_consumed"][i])) == (n, cons), what
                assert blob[at:at + len(out)].tobytes() == out, what
                assert b.output(i, moved=True) == out, what
            at += int(min(r["out_len"][i], r["out_cap"][i]))
            i += 1
    assert i == b.n
    assert b.unwritten_intact(), "bytes outside the jobs' outputs were written"


@pytest.mark.parametrize("copier,team", [(1, 1), (-1, 1), (1, 0), (-1, 0)])
def test_batch_api_cases(runs, copier, team):
    """The directed runs of the CPU tier and the residue pairs in ONE launch of fewer than 256 jobs (the place-scan cases across tiles:
    test_long_run_across_tiles): deflate_team 1 parses with a team per unit, 0 with one wave;
    lz_copier 1 copies with the workgroup resolver, -1 with the wave copier.  An open unit behind an empty stored block, one that
    ends after a fixed block on a byte, the same one code longer, one with a final block and trailing bytes, a unit that reaches one
    byte in front of itself (SWC_E_REF_TRAP, neighbours correct), a middle unit over capacity (reports the length it needs, its
    successor behind out_cap), empty units, and adjacent units at all 16 residues.  Without the feature an open unit ends with
    SWC_E_REF_TRAP."""
    lib = _lib.load()
    units = [u for _, run, _ in runs for u in run]
    assert lib.swc_set_tuning(b"lz_copier", copier) == 0 and lib.swc_set_tuning(b"deflate_team", team) == 0
    try:
        b = DeviceBatch("deflate", [u["data"] for u in units], [u["cap"] for u in units], aux=[u["aux"] for u in units], guard=16)
        assert b.n < 256
        b.launch(sync=True)
        check_batch(b, runs)
        by = {name: exp for name, _, exp in runs}
        assert by["reaches-back"][1][0] == K.REF_TRAP and by["over-capacity"][1][:2] == (K.CAPACITY, 1501)
    finally:
        lib.swc_set_tuning(b"lz_copier", 1)
        lib.swc_set_tuning(b"deflate_team", 1)


def test_joined_job_0(runs):
    """SWC_DEFLATE_JOINED on job 0 and on what is joined to it: SWC_E_INVALID_ARGUMENT, nothing produced, nothing written; the run
    behind them is the oracle's."""
    name, run, exp = runs[0]
    orphans = [dict(run[1]), dict(run[2])]
    units = orphans + run
    b = DeviceBatch("deflate", [u["data"] for u in units], [u["cap"] for u in units], aux=[u["aux"] for u in units], guard=16)
    b.launch(sync=True)
    r = b.results()
    for i in range(2):
        assert (int(r["status"][i]), int(r["out_len"][i]), int(r["in_consumed"][i])) == (K.INVALID_ARGUMENT, 0, 0)
    base = b.d_out.data_ptr()
    at = int(b._out_off[2])
    for i, (st, n, cons, aux, out) in enumerate(exp, start=2):
        assert (int(r["status"][i]), int(r["out_len"][i]), int(r["out"][i]) - base) == (st, n, at)
        assert b.output(i, moved=True) == out
        at += n
    assert b.unwritten_intact()


@pytest.mark.parametrize("copier,team", [(1, 1), (-1, 1), (1, 0), (-1, 0)])
def test_long_run_across_tiles(copier, team):
    """The placing scan across tiles on the device: 37 whole streams, then a run of 150 units that starts at job 37, fills tile 1
    without a head and ends in tile 2 (a look-back two tiles deep, a whole-tile sum), sizes unlike capacities -- a unit of 0 bytes,
    one of 1 byte, one over capacity -- so that every joined unit's place differs from where the batch had put it; then a short run.
    Every `out`, every unit's bytes, its CRC-32 from the launch (lz_copier -1: the copy wave's tail, at any byte address), and the
    guards."""
    lib = _lib.load()
    jobs = K.long_run()
    exp = [K.expect(u) for u in jobs]
    assert len(jobs) == 189 and [e[0] for e in exp].count(K.CAPACITY) == 1 and exp[37 + 20][1] == 0 and exp[37 + 70][1] == 1
    assert lib.swc_set_tuning(b"lz_copier", copier) == 0 and lib.swc_set_tuning(b"deflate_team", team) == 0
    try:
        b = DeviceBatch("deflate", [u["data"] for u in jobs], [u["cap"] for u in jobs], aux=[u["aux"] for u in jobs], guard=16)
        preset = b.results()["out"].copy()
        b.crc32_async()
        b.launch(sync=True)
        assert b._crc_current
        runs = [("whole-%d" % i, jobs[i:i + 1], exp[i:i + 1]) for i in range(37)] + [("long", jobs[37:187], exp[37:187]), ("behind", jobs[187:], exp[187:])]
        check_batch(b, runs)
        r = b.results()
        moved = [i for i in range(b.n) if int(r["out"][i]) != int(preset[i])]
        assert len(moved) >= 140 and set(moved) <= set(range(38, 187)) | {188}      # the scan placed them, not the batch's layout
        crcs = b._crc_buf.cpu().numpy().view(np.uint32)
        assert (crcs == b.crc32()).all()
        for i, (st, n, cons, aux, out) in enumerate(exp):
            assert int(crcs[i]) == zlib.crc32(out), i
        assert len({int(r["out"][i]) % 16 for i in range(37, 187)}) == 16          # ... at every residue
    finally:
        lib.swc_set_tuning(b"lz_copier", 1)
        lib.swc_set_tuning(b"deflate_team", 1)


@pytest.mark.parametrize("copier,team", [(1, 1), (-1, 1), (1, 0), (-1, 0)])
def test_many_runs(copier, team):
    """2,600 runs of three units of 1 KiB: the wave copier (and the launch order) over 7,800 jobs, the CRC-32 of every unit from the
    copy wave's tail; the units' CRCs combine to zlib.crc32 of the run."""
    lib = _lib.load()
    import random
    distinct, want = [], []
    for c in range(16):
        rnd = random.Random(900 + c)
        p = [K.repetitive(rnd, 1024) for _ in range(3)]
        distinct.append([K.U(K.unit_open_stored(p[0]), 1024, K.OPEN), K.U(K.unit_open_stored(p[1]), 1024, K.JOINED | K.OPEN),
                         K.U(K.unit_final(p[2]), 1024, K.JOINED)])
        assert O.deflate(b"".join(u["data"] for u in distinct[-1])) [:2] == (0, b"".join(p))     # the run IS one stream
        want.append(b"".join(p))
    reps = 2600
    jobs = [u for r in range(reps) for u in distinct[r % 16]]
    assert lib.swc_set_tuning(b"lz_copier", copier) == 0 and lib.swc_set_tuning(b"deflate_team", team) == 0
    try:
        b = DeviceBatch("deflate", [u["data"] for u in jobs], [1024] * len(jobs), aux=[u["aux"] for u in jobs], guard=16)
        assert b.n == 7800
        b.crc32_async()          # (allocates the CRC buffer: the launch below leaves the CRCs in it)
        b.launch(sync=True)
        assert b._crc_current
        r = b.results()
        assert (r["status"] == 0).all() and (r["out_len"] == 1024).all()
        assert (r["aux"] == np.tile(np.array([K.OPEN, K.JOINED | K.OPEN, K.JOINED], dtype=np.int32), reps)).all()
        assert (r["out"] - np.uint64(b.d_out.data_ptr()) == b._out_off.astype(np.uint64)).all()      # 1 KiB each: nothing moved
        heads = b._out_off[0::3].astype(np.int64)                                                      # (16 guard bytes in front of every run)
        blob = b.d_out.cpu().numpy()[heads[:, None] + np.arange(3072, dtype=np.int64)[None, :]]
        assert b.unwritten_intact()
        for c in range(16):
            assert (blob[c::16] == np.frombuffer(want[c], dtype=np.uint8)).all(), "run %d" % c
        crcs = b._crc_buf.cpu().numpy().view(np.uint32).reshape(reps, 3)
        assert (crcs == b.crc32().reshape(reps, 3)).all()
        for c in range(16):
            x = 0
            for k in range(3):
                x = lib.swc_crc32_combine(x, int(crcs[c][k]), 1024)
            assert x == zlib.crc32(want[c]) and (crcs[c::16] == crcs[c]).all()
    finally:
        lib.swc_set_tuning(b"lz_copier", 1)
        lib.swc_set_tuning(b"deflate_team", 1)


# ------------------------------------------------------------------------------------------------------------- host paths
def call(name, data, consumed=False, multi=False):
    """An entry point as the C ABI returns it: (status, bytes[, in_consumed]) or (status, [bytes])."""
    lib = _lib.load()
    data = bytes(data)
    out, n, cons = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_size_t()
    if multi:
        sizes, cnt = C.POINTER(C.c_size_t)(), C.c_size_t()
        st = getattr(lib, name)(data, len(data), C.byref(out), C.byref(n), C.byref(sizes), C.byref(cnt))
        blob = C.string_at(out, n.value) if n.value else b""
        szs = [sizes[i] for i in range(cnt.value)]
        lib.swc_free(out)
        lib.swc_free(sizes)
        parts, o = [], 0
        for s in szs:
            parts.append(blob[o:o + s])
            o += s
        return st, parts
    args = [data, len(data), C.byref(out), C.byref(n)] + ([C.byref(cons)] if consumed else [])
    st = getattr(lib, name)(*args)
    blob = C.string_at(out, n.value) if n.value else b""
    lib.swc_free(out)
    return (st, blob, cons.value) if consumed else (st, blob)


class Stats:
    def __init__(self):
        self.lib = _lib.load()
        self.at = self.read()

    def read(self):
        return [self.lib.swc_stat(k) for k in (b"launches", b"units", b"deflate_unit_fallbacks")]

    def delta(self):
        now = self.read()
        d = [a - b for a, b in zip(now, self.at)]
        self.at = now
        return d


@pytest.fixture
def tiny_units():
    lib = _lib.load()
    assert lib.swc_set_tuning(b"deflate_unit_bytes", 1) == 0
    try:
        yield
    finally:
        lib.swc_set_tuning(b"deflate_unit_bytes", DEFAULT_UNIT_BYTES)


def flushed(parts, mode=zlib.Z_FULL_FLUSH, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return b"".join(c.compress(p) + c.flush(mode) for p in parts[:-1]) + c.compress(parts[-1]) + c.flush()


def gzip_of(raw, plain, crc=None):
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", zlib.crc32(plain) if crc is None else crc, len(plain) & 0xFFFFFFFF)


@pytest.fixture(scope="module")
def big():
    return corpus.p_text(5 * (1 << 20) + 12345, 77)


@pytest.fixture
def units_32k():
    lib = _lib.load()
    assert lib.swc_set_tuning(b"deflate_unit_bytes", 32768) == 0
    try:
        yield
    finally:
        lib.swc_set_tuning(b"deflate_unit_bytes", DEFAULT_UNIT_BYTES)


def test_own_archives_come_back_in_one_launch(big, units_32k):
    """Deflate.compress / GzipArchive.archive / ZlibArchive.archive of 5 MiB + 12,345 bytes (21 segments joined by empty stored
    blocks) decode back as units of at least 32,768 bytes: one launch, at least 20 units more, no fallback."""
    s = Stats()
    for make, back in ((swc.Deflate.compress, swc.Deflate.decompress), (swc.GzipArchive.archive, swc.GzipArchive.unarchive),
                       (swc.ZlibArchive.archive, swc.ZlibArchive.unarchive)):
        z = make(big)
        s.delta()
        assert back(z) == big
        launches, units, fallbacks = s.delta()
        print("launches %d units %d fallbacks %d" % (launches, units, fallbacks))
        assert launches == 1 and units >= 20 and fallbacks == 0


def test_knob_zero_is_the_parent(big):
    lib = _lib.load()
    z = swc.GzipArchive.archive(big[:(1 << 20) + 300000])
    assert lib.swc_set_tuning(b"deflate_unit_bytes", 0) == 0
    try:
        s = Stats()
        assert swc.GzipArchive.unarchive(z) == big[:(1 << 20) + 300000]
        launches, units, fallbacks = s.delta()
        assert units == launches and fallbacks == 0      # one unit per launch, as ever (a second launch where the first lacked room)
    finally:
        lib.swc_set_tuning(b"deflate_unit_bytes", DEFAULT_UNIT_BYTES)


def test_shipped_default_never_cuts(big):
    """As shipped the knob is 0: a segmented archive is one unit per launch, as on the parent."""
    z = swc.ZlibArchive.archive(big[:(1 << 20) + 5])
    s = Stats()
    assert swc.ZlibArchive.unarchive(z) == big[:(1 << 20) + 5]
    launches, units, fallbacks = s.delta()
    assert units == launches and fallbacks == 0
    assert swc.index_blocks("deflate", z[2:-4]) == [(0, len(z) - 6, 0, 0)]


def test_full_flush_stream(tiny_units):
    """Z_FULL_FLUSH, four units: the oracle's bytes and in_consumed (trailing bytes behind the stream stay unread), one launch."""
    parts = [corpus.p_text(n, 80 + i) for i, n in enumerate((30000, 7, 50001, 1234))]
    raw = flushed(parts) + b"behind the stream"
    assert len(swc.index_blocks("deflate", flushed(parts))) == 4
    s = Stats()
    assert call("swc_deflate_decompress", raw, consumed=True) == O.deflate(raw) == (0, b"".join(parts), len(raw) - 17)
    assert s.delta() == [1, 4, 0]      # (the bytes behind the stream hold no marker: they belong to the fourth unit)


def test_sync_flush_stream_falls_back(tiny_units):
    """Z_SYNC_FLUSH: the units refer to each other's bytes, so the run does not stand; the stream is decoded whole: the oracle's bytes,
    one fallback."""
    base = corpus.p_text(20000, 90)
    parts = [base, base[5000:15000] + b"!", base[::-1][:3000] + base[:9000]]
    raw = flushed(parts, zlib.Z_SYNC_FLUSH)
    s = Stats()
    assert call("swc_deflate_decompress", raw, consumed=True) == O.deflate(raw) == (0, b"".join(parts), len(raw))
    launches, units, fallbacks = s.delta()
    assert fallbacks == 1 and launches == 2
    z = gzip_of(raw, b"".join(parts))
    assert call("swc_gzip_unarchive", z) == O.gzip_unarchive(z) == (0, b"".join(parts))


def test_markers_inside_stored_data(tiny_units):
    """A stored block full of 00 00 FF FF: every cut is false; the oracle's result through the fallback."""
    w = DB.BitWriter()
    DB.fixed_block(w, list(b"in front "), False)
    DB.stored_block(w, b"\x00\x00\xff\xff" * 2000, False)
    DB.fixed_block(w, list(b" behind"), True)
    raw = w.data()
    s = Stats()
    got = call("swc_deflate_decompress", raw, consumed=True)
    assert got == O.deflate(raw) and got[0] == 0 and len(got[1]) == 9 + 8000 + 7
    assert s.delta()[2] == 1


def test_stream_that_closes_with_an_empty_final_block(tiny_units):
    """... 00 00 FF FF | 01 00 00 FF FF: the marker of the closing block itself is at the very end and cuts nothing; the closing
    block is the last unit, five bytes that decode to nothing."""
    parts = [corpus.p_text(9000, 95), corpus.p_text(4000, 96)]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b"".join(c.compress(p) + c.flush(zlib.Z_FULL_FLUSH) for p in parts) + b"\x01\x00\x00\xff\xff"
    refs = swc.index_blocks("deflate", raw)
    assert [r[3] for r in refs] == [K.OPEN, K.JOINED | K.OPEN, K.JOINED] and refs[-1][:2] == (len(raw) - 5, 5)
    s = Stats()
    assert call("swc_deflate_decompress", raw, consumed=True) == O.deflate(raw) == (0, b"".join(parts), len(raw))
    assert s.delta() == [1, 3, 0]
    za = b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(b"".join(parts)))
    assert call("swc_zlib_unarchive", za) == O.zlib_unarchive(za) == (0, b"".join(parts))
    zb = za[:-1] + bytes([za[-1] ^ 1])
    assert call("swc_zlib_unarchive", zb) == O.zlib_unarchive(zb)


def test_damaged_flushed_member(tiny_units):
    """A flushed gzip member truncated at every 997th byte, and one with a wrong CRC: the oracle's status and output each time."""
    parts = [corpus.p_text(n, 100 + i) for i, n in enumerate((9000, 14000, 5000))]
    plain = b"".join(parts)
    z = gzip_of(flushed(parts), plain)
    assert call("swc_gzip_unarchive", z) == O.gzip_unarchive(z) == (0, plain)
    for cut in range(997, len(z), 997):
        assert call("swc_gzip_unarchive", z[:cut]) == O.gzip_unarchive(z[:cut]), "truncated at %d" % cut
    bad = gzip_of(flushed(parts), plain, crc=zlib.crc32(plain) ^ 0x10)
    got = call("swc_gzip_unarchive", bad)
    assert got == O.gzip_unarchive(bad) and got[0] == 605 and got[1] == plain


def test_multi_and_many(tiny_units):
    """Two flushed members through swc_gzip_multi_unarchive; swc_unarchive_many('gzip', [flushed, plain, flushed with a wrong CRC]) in
    one launch, and the same set as zlib and raw streams."""
    pa = [corpus.p_text(n, 110 + i) for i, n in enumerate((8000, 12000))]
    pb = [corpus.p_text(n, 120 + i) for i, n in enumerate((100, 6000, 30000))]
    a, b = gzip_of(flushed(pa), b"".join(pa)), gzip_of(flushed(pb), b"".join(pb))
    assert call("swc_gzip_multi_unarchive", a + b, multi=True) == O.gzip_multi_unarchive(a + b) == (0, [b"".join(pa), b"".join(pb)])
    plain = corpus.gzip_member(corpus.p_text(20000, 130))
    damaged = gzip_of(flushed(pb), b"".join(pb), crc=1)
    s = Stats()
    got = swc.unarchive_many("gzip", [a, plain, damaged])
    assert s.delta() == [1, 2 + 1 + 3, 0]
    assert got == [O.gzip_unarchive(x) for x in (a, plain, damaged)] and [g[0] for g in got] == [0, 0, 605]
    raws = [flushed(pa), zlib.compress(b"".join(pb))[2:-4], flushed(pb)[:-3]]
    got = swc.unarchive_many("deflate", raws)
    exp = [O.deflate(x) for x in raws]
    assert got == [(st, out if st == 0 else b"") for st, out, _ in exp] and exp[2][0] != 0
    zs = [b"\x78\x9c" + flushed(pa) + struct.pack(">I", zlib.adler32(b"".join(pa))), zlib.compress(b"".join(pb))]
    assert swc.unarchive_many("zlib", zs) == [O.zlib_unarchive(x) for x in zs]
