"""GPU tier of the Deflate units that share history (SWC_DEFLATE_LINKED): the case lists of the CPU tier (_deflate_linked_cases) in one
launch through swc_batch_decompress_ws and swc_batch_decompress_crc32_ws on the MI355X -- with a team per unit and the small-launch
arrangement of phase 2, with one wave per unit and the wave copier over 2,600 jobs, and with the wave copier forced -- and zlib's
own sync-flushed output through the single-shot entry points against the knob-off result and the oracle."""
import struct
import zlib

import numpy as np
import pytest

import _deflate_build as DB
import _deflate_linked_cases as L
import _deflate_units_cases as K
import _oracle as O
import swcompression_amd as swc
from swcompression_amd import _lib
from swcompression_amd.batch import DeviceBatch
from test_gpu_deflate_units import Stats, call, gzip_of

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- batch API
@pytest.fixture(scope="module")
def cases():
    """[(name, units, expected per unit)] in job order -- the reference, computed once: the linked jobs nobody heads first (job 0),
    the directed runs, the sixteen residues, whole streams up to job 60 of a tile, then the chain of seventy tiny units."""
    out = [("linked-job-0", L.linked_job_0(), L.expect(L.linked_job_0()))]
    out += [(name, run, L.expect(run)) for name, run in L.directed_runs().items()]
    out += [("residue-%d" % r, run, L.expect(run)) for r, run in enumerate(L.residue_runs())]
    tiles = L.tiles_run()
    n = sum(len(run) for _, run, _ in out)
    for i in range((60 - n) % 64):
        out.append(("whole-%d" % i, tiles[i:i + 1], [K.expect(dict(tiles[i], open_plain=None))[:5]]))
    n = sum(len(run) for _, run, _ in out)
    assert n % 64 == 60 and n + 70 < 256        # the chain crosses two borders of the placing scan's tiles
    out.append(("seventy-tiny-units", tiles[60:], L.expect(tiles[60:])))
    return out


def check_batch(b, cases, crcs=None):
    r = b.results()
    blob = b.d_out.cpu().numpy()
    base = b.d_out.data_ptr()
    i = 0
    for name, run, exp in cases:
        at = None
        for k, (u, (st, n, cons, aux, out)) in enumerate(zip(run, exp)):
            what = "%s unit %d" % (name, k)
            assert int(r["status"][i]) == st, what
            assert int(r["aux"][i]) == aux, what + ": aux"
            if not u["aux"] & L.JOINED:
                at = int(b._out_off[i])
            if at is None:                     # joined to nothing
                assert (int(r["out_len"][i]), int(r["in_consumed"][i])) == (0, 0), what
                if crcs is not None:
                    assert int(crcs[i]) == 0, what + ": CRC-32"
                i += 1
                continue
            assert int(r["out"][i]) - base == at, what + ": `out` is not behind the predecessor's output"
            made = int(min(r["out_len"][i], r["out_cap"][i]))
            if n is not None:
                assert (int(r["out_len"][i]), int(r["in_consumed"][i])) == (n, cons), what
            if out is not None:
                assert blob[at:at + made].tobytes() == out, what
            if crcs is not None:
                assert int(crcs[i]) == zlib.crc32(blob[at:at + made].tobytes()), what + ": CRC-32"
            at += made
            i += 1
    assert i <= b.n
    assert b.unwritten_intact(), "bytes outside the jobs' outputs were written"


def launch_and_check(cases, pad_to=0, crc=False):
    units = [u for _, run, _ in cases for u in run]
    pad = []
    if pad_to > len(units):                   # whole streams behind the cases: the launch reaches the wave copier's threshold
        whole = L.tiles_run()[:60]
        pad = [whole[i % 60] for i in range(pad_to - len(units))]
    jobs = units + pad
    b = DeviceBatch("deflate", [u["data"] for u in jobs], [u["cap"] for u in jobs], aux=[u["aux"] for u in jobs], guard=16)
    if crc:
        b.crc32_async()          # (allocates the CRC buffer: the launch below leaves the CRCs in it)
    b.launch(sync=True)
    crcs = None
    if crc:
        assert b._crc_current
        crcs = b._crc_buf.cpu().numpy().view(np.uint32)
    check_batch(b, cases, crcs)
    if pad:
        r = b.results()
        assert (r["status"][len(units):] == 0).all()
        want = [K.expect(dict(u, open_plain=None))[4] for u in L.tiles_run()[:60]]
        for i in range(len(units), b.n, 97):
            assert b.output(i) == want[(i - len(units)) % 60]
    return b


@pytest.mark.parametrize("crc", [False, True])
@pytest.mark.parametrize("way", ["team", "one-wave-2600", "wave-copier"])
def test_case_lists_in_one_launch(cases, way, crc):
    """Every case of the CPU tier in ONE launch: as is (a team per unit; the resolver skips the chains and the chain kernel copies
    them), with deflate_team = 0 and the list padded with whole streams to 2,600 jobs (one wave per unit, the wave copier and the chain
    kernel behind it), and with lz_copier = -1.  The seam, the overlap across it, the sixteen residues, distance 32,768 with 40,000 and
    with 32,767 bytes in front, a source far in front of the copier's window, a chain that restarts, a predecessor over capacity and a
    failed one, units of 0 and 1 bytes, the bit without JOINED, linked jobs nobody heads, a chain across three tiles.  Without the
    feature the unit behind the seam reports SWC_E_REF_TRAP."""
    lib = _lib.load()
    by = {name: exp for name, _, exp in cases}
    assert by["seam-5-1"][1][0] == L.OK and by["seam-one-more"][1][0] == L.REF_TRAP and by["saturation-trap"][2][0] == L.REF_TRAP
    try:
        if way == "one-wave-2600":
            assert lib.swc_set_tuning(b"deflate_team", 0) == 0
        if way == "wave-copier":
            assert lib.swc_set_tuning(b"lz_copier", -1) == 0
        b = launch_and_check(cases, pad_to=2600 if way == "one-wave-2600" else 0, crc=crc)
        assert b.n == (2600 if way == "one-wave-2600" else sum(len(run) for _, run, _ in cases))
    finally:
        lib.swc_set_tuning(b"lz_copier", 1)
        lib.swc_set_tuning(b"deflate_team", 1)


# ------------------------------------------------------------------------------------------------------------- host paths
@pytest.fixture(scope="module")
def flushed():
    """(raw stream, gzip member, zlib stream, plain): zlib's output, 300,000 bytes of text with Z_SYNC_FLUSH every 40,000."""
    raw, plain = L.sync_flush_stream()
    return raw, gzip_of(raw, plain), b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(plain)), plain


def with_knobs(unit_bytes, linked, fn):
    lib = _lib.load()
    assert lib.swc_set_tuning(b"deflate_unit_bytes", unit_bytes) == 0 and lib.swc_set_tuning(b"deflate_units_linked", linked) == 0
    try:
        return fn()
    finally:
        lib.swc_set_tuning(b"deflate_unit_bytes", 0)
        lib.swc_set_tuning(b"deflate_units_linked", 0)


def test_sync_flushed_stream_decodes_as_units(flushed):
    """deflate_unit_bytes = 32768 and deflate_units_linked = 1: the bytes, in_consumed and the trailer's verdict are the knob-off result
    (and the oracle's), no fallback is counted, and every call is one launch of several units.  Without the feature the stream counts
    a fallback."""
    raw, gz, zl, plain = flushed
    assert len(with_knobs(32768, 1, lambda: swc.index_blocks("deflate", raw))) >= 3
    bad_gz = gzip_of(raw, plain, crc=zlib.crc32(plain) ^ 4)
    bad_zl = zl[:-1] + bytes([zl[-1] ^ 1])
    for name, data, kw in (("swc_deflate_decompress", raw + b"behind", {"consumed": True}), ("swc_gzip_unarchive", gz, {}), ("swc_zlib_unarchive", zl, {}),
                           ("swc_gzip_unarchive", bad_gz, {}), ("swc_zlib_unarchive", bad_zl, {})):
        off = with_knobs(0, 0, lambda: call(name, data, **kw))
        s = Stats()
        on = with_knobs(32768, 1, lambda: call(name, data, **kw))
        launches, units, fallbacks = s.delta()
        assert on == off, name
        assert on[1] == plain and (on[0] == 0) == (data not in (bad_gz, bad_zl)), name
        assert fallbacks == 0 and launches == 1 and units >= 3, (name, launches, units, fallbacks)
    assert call("swc_deflate_decompress", raw, consumed=True) == O.deflate(raw) == (0, plain, len(raw))
    assert call("swc_gzip_unarchive", bad_gz) == O.gzip_unarchive(bad_gz)


def test_unarchive_many(flushed):
    raw, gz, zl, plain = flushed
    other = zlib.compress(plain[:50000])
    for kind, items in (("deflate", [raw, other[2:-4]]), ("gzip", [gz, gzip_of(other[2:-4], plain[:50000])]), ("zlib", [zl, other])):
        off = with_knobs(0, 0, lambda: swc.unarchive_many(kind, items))
        s = Stats()
        on = with_knobs(32768, 1, lambda: swc.unarchive_many(kind, items))
        launches, units, fallbacks = s.delta()
        assert on == off and [x[0] for x in on] == [0, 0] and on[0][1] == plain, kind
        assert fallbacks == 0 and launches == 1 and units >= 4, (kind, launches, units, fallbacks)


def test_false_marker_still_falls_back():
    """A stored block full of 00 00 FF FF inside a sync-flushed stream: a cut inside stored data is false, the run does not stand, the
    stream is decoded whole and the result is the reference's."""
    w = DB.BitWriter()
    DB.fixed_block(w, list(b"in front "), False)
    DB.stored_block(w, b"", False)
    DB.fixed_block(w, [(5, 4)] + list(b" reaches back "), False)
    DB.stored_block(w, b"\x00\x00\xff\xff" * 500, False)
    DB.fixed_block(w, [(9, 2000)] + list(b" behind"), True)
    raw = w.data()
    s = Stats()
    got = with_knobs(1, 1, lambda: call("swc_deflate_decompress", raw, consumed=True))
    assert got == O.deflate(raw) and got[0] == 0 and len(got[1]) == 9 + 5 + 14 + 2000 + 9 + 7
    assert s.delta()[2] == 1
