"""GPU tier of the LZMA2 units: streams cut at their dictionary resets (include/swc_hip.h: SWC_LZMA2_OPEN, swc_index_blocks kind 8,
"lzma2_run_bytes") through the batch API and through every host path that decodes LZMA2, on the MI355X, against the oracle and
the expectations of the stream builder.  Every stream has at most 8 runs of at most 64 KiB."""
import functools
import random
import struct
import zlib

import pytest

import _emu_lzma2_runs as R
import _lzma_build as B
import _oracle as O
import _xz_build as X
import swcompression_amd as swc
from swcompression_amd import _lib
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu

OPEN, DB = DeviceBatch.LZMA2_OPEN, R.RECIPE_DICT_BYTE
MANY_RESETS = "dictionary-reset-0xE0-mid-stream-64-times"
BEHIND_RESET = "match-reaching-behind-a-dictionary-reset"


class Stats:
    KEYS = (b"launches", b"units", b"lzma2_run_units", b"lzma2_run_fallbacks", b"xz_cache_hits")

    def __init__(self):
        self.lib = _lib.load()
        self.at = self.read()

    def read(self):
        return [self.lib.swc_stat(k) for k in self.KEYS]

    def delta(self):
        """(launches, units, run units, fallbacks, cache hits) since the last call."""
        now = self.read()
        d = tuple(b - a for a, b in zip(self.at, now))
        self.at = now
        return d


KEY = [0]   # "lzma2_run_bytes" as the test in progress wants it (the library has no getter)


@pytest.fixture
def runs_on():
    """The key at 1 for the test, 0 again behind it."""
    lib = _lib.load()
    assert lib.swc_set_tuning(b"lzma2_run_bytes", 1) == 0
    KEY[0] = 1
    yield lib
    KEY[0] = 0
    lib.swc_set_tuning(b"lzma2_run_bytes", 0)


def with_key(key, fn):
    """fn() with the key at `key`; afterwards the key is what the test in progress wants."""
    lib = _lib.load()
    assert lib.swc_set_tuning(b"lzma2_run_bytes", key) == 0
    try:
        return fn()
    finally:
        lib.swc_set_tuning(b"lzma2_run_bytes", KEY[0])


def units_of(chunks, dict_byte):
    """swc_index_blocks kind 8 with the key at 1: (offset from the first chunk, comp_len, uncomp_len, aux)."""
    return with_key(1, lambda: [(off - 1, comp, uncomp, aux) for off, comp, uncomp, aux in
                                swc.index_blocks("lzma2_runs", bytes([dict_byte]) + bytes(chunks))])


@functools.lru_cache(maxsize=None)
def directed():
    """The directed LZMA2 cases and the oracle's word on them, computed once; each held to the kind of result it was built for."""
    cases = [c for c in B.directed_cases() if c.kind == "lzma2"]
    exp = [O.lzma2(c.stream, c.dict_byte) for c in cases]
    for c, e in zip(cases, exp):
        assert e == (0, c.plain, c.consumed) if c.status == 0 else e[0] == c.status, c.name
    return cases, exp


@functools.lru_cache(maxsize=None)
def recipe_stream(runs=6, seed=0, shape=(3, 0, 2)):
    """`runs` parts at positions that are multiples of 16 (the last part odd), 64 KiB the largest: (parts, chunks)."""
    sizes = [65536, 4112, 16, 30000, 48, 12000, 1600, 800][:runs - 1] + [3001]
    parts = [R.text(n, 1000 * seed + i) for i, n in enumerate(sizes)]
    z = R.recipe(parts, shape)
    assert len(units_of(z, DB)) == runs
    return parts, z


def single(chunks, dict_byte):
    """swc_lzma2_decompress: (status, bytes, in_consumed) -- an error carries nothing."""
    try:
        out, cons = swc.LZMA2.decompress_raw(chunks, dict_byte)
        return 0, out, cons
    except swc.SWCError as e:
        return e.status, b"", None


def single_data(chunks, dict_byte):
    """swc_lzma2_decompress_data: (status, bytes)."""
    try:
        return 0, swc.LZMA2.decompress(bytes([dict_byte]) + bytes(chunks))
    except swc.SWCError as e:
        return e.status, b""


# ------------------------------------------------------------------------------------------------------------- device-resident
@pytest.mark.parametrize("coder_cache", [1, 0], ids=["coder-cache", "coders-in-lds"])
@pytest.mark.parametrize("workspace", [True, False], ids=["workspace", "no-workspace"])
def test_device_batch_units(workspace, coder_cache):
    """The units kind 8 lists as jobs of one launch, IN PLACE: every stream lies once in HBM, in an allocation of its own length, and
    a unit is a sub-range of it with the next run's control byte right behind.  Outputs adjacent in one buffer with a guard byte in
    front of every unit and behind the last (an odd dictionary byte among them: bit 0 of an LZMA2 aux is no link); every unit but the
    last of a stream ends open at its last byte, the last meets the end marker with the bit cleared."""
    import numpy as np
    import torch
    lib = _lib.load()
    cases, _ = directed()
    many = next(c for c in cases if c.name == MANY_RESETS)
    parts, z = recipe_stream()
    parts3, z3 = recipe_stream(3, 5)
    streams = [(z, DB, b"".join(parts)), (many.stream, many.dict_byte, many.plain), (z3, DB + 1, b"".join(parts3))]
    units, caps, aux, owner, offs = [], [], [], [], []
    for s, (chunks, db, plain) in enumerate(streams):
        refs = units_of(chunks, db)
        assert 3 <= len(refs) <= 8 and sum(u for _, _, u, _ in refs) == len(plain)
        for k, (off, comp, uncomp, a) in enumerate(refs):
            assert a == db | (OPEN if k + 1 < len(refs) else 0)
            units.append(chunks[off:off + comp]); caps.append(uncomp); aux.append(a); owner.append(s); offs.append(off)
    try:
        assert lib.swc_set_tuning(b"lzma_coder_cache", coder_cache) == 0
        b = DeviceBatch("lzma2", units, caps, aux=aux, guard=1)
        staged = [torch.from_numpy(np.frombuffer(chunks, dtype=np.uint8).copy()).to(b.device) for chunks, _, _ in streams]
        jobs = b._jobs_host.copy()
        for i in range(len(units)):
            jobs["in"][i] = staged[owner[i]].data_ptr() + offs[i]
        b.d_jobs.copy_(torch.from_numpy(jobs.view(np.uint8)).to(b.device))
        if not workspace:
            b.ws_bytes = 0
        b.launch(sync=True)
        r = b.results()
    finally:
        lib.swc_set_tuning(b"lzma_coder_cache", 1)
    for i in range(len(units)):
        assert int(r["in"][i]) == staged[owner[i]].data_ptr() + offs[i]
        assert int(r["status"][i]) == 0, i
        assert int(r["aux"][i]) == aux[i], "unit %d: the OPEN bit stays where the unit ended open, and only there" % i
        assert int(r["in_consumed"][i]) == len(units[i]) and int(r["out_len"][i]) == caps[i], i
        assert b.d_out[b.out_offset(i) + int(b._out_off[i]) - 1].item() == 0xA5, "unit %d: no guard byte in front" % i
    for s, (_, _, plain) in enumerate(streams):
        assert b"".join(b.output(i, caps[i]) for i in range(len(units)) if owner[i] == s) == plain
    assert b.unwritten_intact()


# ----------------------------------------------------------------------------------------------------------------- single shot
def test_single_shot_directed():
    """swc_lzma2_decompress and swc_lzma2_decompress_data over every directed case: the key at 1 gives what the key at 0 gives and
    what the oracle expects -- status, bytes, in_consumed; the counters move on the streams that are cut, and only there."""
    cases, exp = directed()
    s = Stats()
    for c, e in zip(cases, exp):
        n_units = len(units_of(c.stream, c.dict_byte))
        off = with_key(0, lambda: single(c.stream, c.dict_byte))
        launches, units, run_units, fallbacks, _ = s.delta()
        assert launches == units and (run_units, fallbacks) == (0, 0), c.name      # (lc + lp > 4: once more with a workspace)
        on = with_key(1, lambda: single(c.stream, c.dict_byte))
        _, _, run_units, fallbacks, _ = s.delta()
        on_data = with_key(1, lambda: single_data(c.stream, c.dict_byte))
        s.delta()
        want = (0, e[1], e[2]) if e[0] == 0 else (e[0], b"", None)
        assert off == want and on == want and on_data == want[:2], c.name
        if n_units < 2:
            assert (run_units, fallbacks) == (0, 0), c.name
        else:
            assert (run_units, fallbacks) in ((n_units, 0), (0, 1)), c.name
        if c.name == MANY_RESETS:
            assert n_units == 8 and (run_units, fallbacks) == (8, 0)
        if c.name == BEHIND_RESET:            # (its reset lies at 100, no multiple of 16: not cut -- the aligned twin is below)
            assert n_units == 1


def test_single_shot_random():
    rnd = random.Random(0x12A2D00)
    cases = []
    while len(cases) < 100:
        c = B.random_stream(rnd, rnd.choice([1, 9, 300, 4000, 20000]), len(cases) % 2 == 0)
        if c.kind == "lzma2":
            cases.append(c)
    s = Stats()
    accepted = 0
    for i, c in enumerate(cases):
        want = (0, c.plain, c.consumed)
        assert with_key(0, lambda: single(c.stream, c.dict_byte)) == want, i
        # what the host emulation of the same kernel makes of the units decides what the counters must show
        refs = units_of(c.stream, c.dict_byte)
        expect = (0, 0)
        if len(refs) >= 2:
            ok = R.accept(refs, R.run_jobs(c.stream, refs, 0)) is not None
            expect = (len(refs), 0) if ok else (0, 1)
            accepted += ok
        s.delta()
        assert with_key(1, lambda: single(c.stream, c.dict_byte)) == want, i
        assert s.delta()[2:4] == expect, i
        assert with_key(1, lambda: single_data(c.stream, c.dict_byte)) == want[:2], i
    assert accepted >= 1


def test_fallbacks_report_the_whole_stream(runs_on):
    """A match that reaches behind a reset -- legal in the stream, a failure in the unit -- and a byte corrupted in the second run:
    the stream is decoded whole and THAT result is the call's."""
    s = Stats()
    c = R.aligned_match_behind_reset()
    assert len(units_of(c.stream, c.dict_byte)) == 2 and O.lzma2(c.stream, c.dict_byte) == (0, c.plain, c.consumed)
    s.delta()
    assert single(c.stream, c.dict_byte) == (0, c.plain, c.consumed)
    assert s.delta()[:4] == (2, 3, 0, 1)
    parts, z = recipe_stream()
    refs = units_of(z, DB)
    bad = bytearray(z)
    bad[refs[1][0] + refs[1][1] // 2] ^= 0x10
    want = O.lzma2(bytes(bad), DB)
    assert want[0] != 0
    s.delta()
    assert single(bytes(bad), DB)[0] == want[0]
    assert s.delta()[:4] == (2, len(refs) + 1, 0, 1)
    assert single_data(bytes(bad), DB)[0] == want[0]
    # cut one byte short in the last run, and with the end marker gone
    for damaged in (z[:-2], z[:-1]):
        assert single(damaged, DB)[0] == O.lzma2(damaged, DB)[0] != 0


def test_aligned_stored_reset_with_the_model_going_on(runs_on):
    """A stored dictionary reset at a multiple of 16 with 0x80 / 0xA0 / 0x02 then 0x80 behind it is no cut: the stream is cut at its
    later 0xE0 alone, both units are accepted, and the result is the stream's."""
    s = Stats()
    for c, _ in R.aligned_stored_resets():
        assert len(units_of(c.stream, c.dict_byte)) == 2, c.name
        s.delta()
        assert single(c.stream, c.dict_byte) == (0, c.plain, c.consumed), c.name
        assert s.delta()[:4] == (1, 2, 2, 0), c.name
        assert single_data(c.stream, c.dict_byte) == (0, c.plain), c.name


def test_key_0_is_the_parent_path():
    """With the key at 0 a stream of many runs is one unit of one launch, as ever."""
    parts, z = recipe_stream()
    s = Stats()
    assert single(z, DB) == (0, b"".join(parts), len(z))
    assert s.delta()[:4] == (1, 1, 0, 0)
    assert swc.unarchive_many("lzma2", [bytes([DB]) + z] * 3) == [(0, b"".join(parts))] * 3
    assert s.delta()[:4] == (1, 3, 0, 0)


def test_runs_share_one_launch(runs_on):
    parts, z = recipe_stream()
    s = Stats()
    assert single(z, DB) == (0, b"".join(parts), len(z))
    assert s.delta()[:4] == (1, 6, 6, 0)


# --------------------------------------------------------------------------------------------------------------------- .xz
def xz_single_block(blocks, check):
    """An .xz stream framed by hand around given LZMA2 payloads (tests/_xz_build.py has the fields): blocks = [(chunks, plain)],
    the dictionary byte of recipe().  Returns (stream, offsets of the check fields)."""
    flags = bytes([0, check])
    out = bytearray(b"\xFD7zXZ\x00" + flags + struct.pack("<I", zlib.crc32(flags) & 0xFFFFFFFF))
    records, checks = [], []
    for comp, plain in blocks:
        body = bytes([0xC0]) + X.multibyte(len(comp)) + X.multibyte(len(plain)) + X.multibyte(0x21) + X.multibyte(1) + bytes([DB])
        body += X._pad4(1 + len(body))
        header = bytes([(1 + len(body) + 4) // 4 - 1]) + body
        header += struct.pack("<I", zlib.crc32(header) & 0xFFFFFFFF)
        out += header + comp + X._pad4(len(comp))
        field = X.check_field(check, plain)
        checks.append(len(out))
        out += field
        records.append((len(header) + len(comp) + len(field), len(plain)))
    index = b"\x00" + X.multibyte(len(records)) + b"".join(X.multibyte(a) + X.multibyte(b) for a, b in records)
    index += X._pad4(len(index))
    index += struct.pack("<I", zlib.crc32(index) & 0xFFFFFFFF)
    out += index
    tail = struct.pack("<I", len(index) // 4 - 1) + flags
    out += struct.pack("<I", zlib.crc32(tail) & 0xFFFFFFFF) + tail + b"YZ"
    return bytes(out), checks


@pytest.mark.parametrize("check", [X.CHECK_CRC32, X.CHECK_CRC64, X.CHECK_SHA256], ids=["crc32", "crc64", "sha256"])
def test_xz_single_block_of_six_runs(runs_on, check):
    parts, z = recipe_stream()
    plain = b"".join(parts)
    xz, checks = xz_single_block([(z, plain)], check)
    assert O.xz_unarchive(xz) == (0, plain)
    s = Stats()
    assert swc.XZArchive.unarchive(xz) == plain
    assert s.delta()[:4] == (1, 6, 6, 0)
    bad = bytearray(xz)
    bad[checks[0]] ^= 1
    with pytest.raises(swc.XZError) as ei:             # a check mismatch still carries the data
        swc.XZArchive.unarchive(bytes(bad))
    assert ei.value.case == "wrongCheck" and ei.value.data == plain
    assert with_key(0, lambda: swc.XZArchive.unarchive(xz)) == plain


@pytest.mark.parametrize("check", [X.CHECK_CRC32, X.CHECK_CRC64], ids=["crc32", "crc64"])
def test_xz_blocks_times_runs_decoded_ahead(runs_on, check):
    """Two blocks of three runs each: blocks x runs in the launch that runs ahead; the device CRC-32 of a block is combined from its
    units', any other check is taken over the joined block -- and either still finds a damaged check."""
    blocks = []
    for seed in (1, 2):
        parts, z = recipe_stream(3, seed)
        blocks.append((z, b"".join(parts)))
    plain = b"".join(p for _, p in blocks)
    xz, checks = xz_single_block(blocks, check)
    assert O.xz_unarchive(xz) == (0, plain)
    s = Stats()
    assert swc.XZArchive.unarchive(xz) == plain
    assert s.delta() == (1, 6, 6, 0, 2)
    bad = bytearray(xz)
    bad[checks[1] + 1] ^= 0x40
    with pytest.raises(swc.XZError) as ei:
        swc.XZArchive.unarchive(bytes(bad))
    assert ei.value.case == "wrongCheck" and ei.value.data == plain


# ---------------------------------------------------------------------------------------------------------- many archives, 7-Zip
def eight_streams(fallback):
    """(chunks, plain) x 8: 1-run and multi-run streams mixed; fallback: one of them is the stream whose unit reaches back."""
    out = []
    for k in range(8):
        runs = [1, 4, 1, 6, 3, 1, 8, 2][k]
        if runs == 1:
            p = R.text(5000 + 16 * k, 50 + k)
            out.append((R.recipe([p]), p))
        else:
            parts, z = recipe_stream(runs, 10 + k, R.SHAPES[k % 4])
            out.append((z, b"".join(parts)))
    if fallback:          # (built for a larger dictionary; its one match reaches 60 bytes back: the same stream under the recipe's byte)
        c = R.aligned_match_behind_reset()
        assert O.lzma2(c.stream, DB) == (0, c.plain, c.consumed)
        out[2] = (c.stream, c.plain)
    return out


@pytest.mark.parametrize("fallback", [False, True], ids=["accepted", "one-falls-back"])
@pytest.mark.parametrize("kind", ["lzma2", "xz"])
def test_unarchive_many(runs_on, kind, fallback):
    streams = eight_streams(fallback)
    counts = [len(units_of(z, DB)) for z, _ in streams]
    assert [c >= 2 for c in counts] == [k not in (0, 5) and (k != 2 or fallback) for k in range(8)]
    accepted = sum(c for k, c in enumerate(counts) if c >= 2 and not (fallback and k == 2))
    if kind == "lzma2":
        archives = [bytes([DB]) + z for z, _ in streams]
    else:
        archives = [xz_single_block([(z, p)], X.CHECK_CRC32)[0] for z, p in streams]
    s = Stats()
    got = swc.unarchive_many(kind, archives)
    launches, units, run_units, fallbacks, _ = s.delta()
    assert got == [(0, p) for _, p in streams]
    assert fallbacks == (1 if fallback else 0) and run_units == accepted
    assert launches <= (3 if fallback else 2)
    assert units == sum(counts) + (1 if fallback else 0)              # the units of every stream, and the fallen-back stream whole


def test_7z_folder_of_four_runs(runs_on):
    from swcompression_amd.sevenzip import SevenZipFolder
    parts, z = recipe_stream(4, 7)
    plain = b"".join(parts)
    chain = [("lzma2", bytes([DB]), len(plain))]
    assert O.sevenzip_folder(z, chain) == (0, plain)
    s = Stats()
    assert SevenZipFolder.unpack_many([(z, chain)]) == [(0, plain)]
    assert s.delta()[:4] == (1, 4, 4, 0)
