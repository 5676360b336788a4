"""CPU tier: LZMA2 streams cut at their dictionary resets -- the SWC_LZMA2_OPEN bit of a job (swcompression_amd/csrc/lzma_wave.h on
the host emulation, both model layouts), swc_index_blocks kind 8, and the units end to end under the acceptance rule of
include/swc_hip.h -- against the oracle and the expectations of the stream builder (tests/_lzma_build.py)."""
import functools
import random

import pytest

import _emu
import _emu_lzma2_runs as R
import _lzma_build as B
import _oracle as O
import swcompression_amd as swc
from swcompression_amd import _lib

OPEN, DB = R.OPEN, R.RECIPE_DICT_BYTE
TRAP = B.TRAP
MODES = pytest.mark.parametrize("mode", [0, 1], ids=["coders-in-lds", "coder-cache"])


def test_open_is_the_documented_bit():
    from swcompression_amd.batch import DeviceBatch
    assert DeviceBatch.LZMA2_OPEN == OPEN == 0x100


def units_of(chunks, dict_byte, key=1):
    """swc_index_blocks kind 8 with "lzma2_run_bytes" = key, offsets counted from the first chunk (as the jobs take them)."""
    lib = _lib.load()
    assert lib.swc_set_tuning(b"lzma2_run_bytes", key) == 0
    try:
        refs = swc.index_blocks("lzma2_runs", bytes([dict_byte]) + bytes(chunks), flags=True)
    finally:
        lib.swc_set_tuning(b"lzma2_run_bytes", 0)
    assert all(f == 0 for *_, f in refs)
    return [(off - 1, comp, uncomp, aux) for off, comp, uncomp, aux, _ in refs]


def check_tiling(refs, chunks, dict_byte):
    """Offsets and sizes tile the stream; every unit but the last is OPEN, all carry the dictionary byte."""
    at = 0
    for k, (off, comp, uncomp, aux) in enumerate(refs):
        assert off == at and comp > 0
        assert aux == (dict_byte | (OPEN if k + 1 < len(refs) else 0))
        at += comp
    assert at == len(chunks)


@functools.lru_cache(maxsize=None)
def two_parts():
    parts = [R.text(4096, 1), R.text(3000, 2)]
    z = R.recipe(parts)
    refs = units_of(z, DB)
    assert len(refs) == 2 and refs[0][2] == 4096
    return parts, z, refs


# ---------------------------------------------------------------------------------------------------------------- the OPEN bit
@MODES
def test_open_unit_ends_at_its_last_byte(mode):
    parts, z, refs = two_parts()
    n = refs[0][1]
    # in place inside the stream: the next run's control byte follows directly
    (st, out, cons, out_len, aux), = R.run_jobs(z, [(0, n, 4096, DB | OPEN)], mode)
    assert (st, out, cons, out_len, aux) == (0, parts[0], n, 4096, DB | OPEN)
    # with the end marker appended the unit ends there like any stream: the bit comes back cleared
    (st, out, cons, out_len, aux), = R.run_jobs(z[:n] + b"\0", [(0, n + 1, 4096, DB | OPEN)], mode)
    assert (st, out, cons, out_len, aux) == (0, parts[0], n + 1, 4096, DB)
    # without the bit the same input ends as ever: the control byte is read past the end, the reference's trap
    (st, out, cons, out_len, aux), = R.run_jobs(z, [(0, n, 4096, DB)], mode)
    assert (st, cons, out_len, aux) == (TRAP, n, 4096, DB) and out == parts[0]
    assert O.lzma2(z[:n], DB)[0] == TRAP


@MODES
def test_nothing_behind_the_unit_matters(mode):
    parts, z, refs = two_parts()
    n = refs[0][1]
    want = R.run_jobs(z, [(0, n, 4096, DB | OPEN)], mode)
    assert z[n] != 0
    for behind in (b"\xFF" * 300, b"\x01\x00", b"\x00", b""):
        assert R.run_jobs(z[:n] + behind, [(0, n, 4096, DB | OPEN)], mode) == want
    # the last unit as well: whatever follows the end marker
    last = refs[1]
    want = R.run_jobs(z, [(last[0], last[1], last[2], DB)], mode)
    assert want[0][:4] == (0, parts[1], last[1], len(parts[1]))
    assert R.run_jobs(z + b"\xE0" * 64, [(last[0], last[1], last[2], DB)], mode) == want


@MODES
def test_errors_are_kept(mode):
    parts, z, refs = two_parts()
    n = refs[0][1]
    # cut one byte short: the last chunk runs past the end
    with_bit, = R.run_jobs(z, [(0, n - 1, 4096, DB | OPEN)], mode)
    without, = R.run_jobs(z, [(0, n - 1, 4096, DB)], mode)
    assert with_bit == without and with_bit[0] == O.lzma2(z[:n - 1], DB)[0] != 0 and with_bit[4] == DB
    # the unit's last LZMA chunk announces one byte more than it holds
    chunks = swc.index_blocks("lzma2", bytes([DB]) + z[:n] + b"\0")
    off = chunks[-1][0] - 1
    assert z[off] >= 0x80 and off + chunks[-1][1] == n
    unpack = ((z[off] & 0x1F) << 16 | z[off + 1] << 8 | z[off + 2]) + 1
    bad = bytearray(z)
    bad[off:off + 3] = bytes([(z[off] & 0xE0) | (unpack >> 16), (unpack >> 8) & 0xFF, unpack & 0xFF])
    with_bit, = R.run_jobs(bad, [(0, n, 4200, DB | OPEN)], mode)
    without, = R.run_jobs(bad, [(0, n, 4200, DB)], mode)
    want = O.lzma2(bytes(bad[:n]), DB)[0]
    assert want not in (0, 901) and with_bit[0] == without[0] == want and with_bit[4] == DB


@MODES
def test_empty_input_keeps_its_status(mode):
    for aux in (DB, DB | OPEN):
        (st, out, cons, out_len, aux_out), = R.run_jobs(b"\xE0", [(0, 0, 16, aux)], mode)
        assert (st, out, cons, out_len) == (O.lzma2(b"", DB)[0], b"", 0, 0) and st == TRAP and aux_out == DB


# ------------------------------------------------------------------------------------------------------------------ index kind 8
def test_index_cuts_where_the_position_is_a_multiple_of_16():
    parts = [R.text(4096, 3), R.text(4112, 4), R.text(33, 5), R.text(1000, 6)]
    z = R.recipe(parts)
    refs = units_of(z, DB, 1)
    check_tiling(refs, z, DB)
    assert [u for _, _, u, _ in refs] == [4096, 4112, 33 + 1000]          # cuts at 4,096 and 8,208, none at 8,241
    for (off, comp, uncomp, aux), want in zip(refs, (parts[0], parts[1], parts[2] + parts[3])):
        assert O.lzma2(z[off:off + comp] + (b"\0" if aux & OPEN else b""), DB)[:2] == (0, want)
    one = units_of(z, DB, 0)                                               # the shipped default: one unit
    assert one == [(0, len(z), sum(len(p) for p in parts), DB)]
    assert units_of(z, DB, 1 << 20) == one                                 # a large key merges everything
    merged = units_of(z, DB, refs[0][1] + 1)                               # ... and a middle one the first two
    check_tiling(merged, z, DB)
    assert [u for _, _, u, _ in merged] == [4096 + 4112, 33 + 1000]
    assert _lib.load().swc_set_tuning(b"lzma2_run_bytes", -1) != 0


def test_index_never_cuts_where_the_model_goes_on():
    by_name = {c.name: c for c in B.directed_cases()}
    for name in ("dictionary-reset-0x01-mid-stream-then-0x80", "0x80-behind-a-stored-chunk-that-reset-the-dictionary"):
        c = by_name[name]
        chunks = swc.index_blocks("lzma2", bytes([c.dict_byte]) + c.stream)
        stored = [off - 1 for off, _, _, control, _ in chunks if control == 1]
        assert stored, name
        refs = units_of(c.stream, c.dict_byte)
        check_tiling(refs, c.stream, c.dict_byte)
        assert not set(stored) & {off for off, _, _, _ in refs}, name
    # a stored reset in front of a chunk that brings state and properties IS a cut, where the position allows it
    b = B._new("lzma2", (3, 0, 2), None)
    for i in range(32):
        b.literal(i)
    b.stored(b"\x11" * 16, True)
    b.chunk(0xC0, (2, 0, 1))
    for i in range(20):
        b.literal(0x40 + i)
    b.stored(b"\x22" * 12, True)      # at 68: not a multiple of 16
    b.chunk(0xE0, (3, 0, 2))          # at 80
    b.literal(7)
    b.stored(b"\x33" * 15, True)      # at 81; behind it the stream ends: a cut but for the position
    c = b.case("stored-resets")
    assert [u for _, _, u, _ in units_of(c.stream, c.dict_byte)] == [32, 16 + 20 + 12, 1 + 15]


@MODES
def test_aligned_stored_reset_with_the_model_going_on_is_no_cut(mode):
    """0x01 at a multiple of 16 followed by 0x80, by 0xA0 under properties that are not the defaults, and by 0x02 then 0x80: only the
    look at the next chunk that is not stored keeps kind 8 from cutting there.  The stream is cut at its later 0xE0 alone, and the
    units give the stream; a unit that began at the stored chunk would not (0xA0: it builds the default model)."""
    for c, at in R.aligned_stored_resets():
        assert O.lzma2(c.stream, c.dict_byte) == (0, c.plain, c.consumed), c.name
        chunks = swc.index_blocks("lzma2", bytes([c.dict_byte]) + c.stream)
        (stored, size), = [(off - 1, uncomp) for off, _, uncomp, control, _ in chunks if control == 1]
        assert at % 16 == 0 and c.plain[at:at + size] == c.stream[stored + 3:stored + 3 + size], c.name
        refs = units_of(c.stream, c.dict_byte)
        check_tiling(refs, c.stream, c.dict_byte)
        assert len(refs) == 2 and c.stream[refs[1][0]] == 0xE0 and refs[0][2] % 16 == 0 and refs[0][2] > at + size, c.name
        n, got = decode_as_units(c.stream, c.dict_byte, mode, (0, c.plain, c.consumed))
        assert n == 2 and got == (c.plain, c.consumed), c.name
        # what the look-ahead prevents: the run from the stored chunk on, decoded on its own, is not what the stream holds there
        alone = R.run_jobs(c.stream, [(stored, refs[1][0] - stored, refs[0][2] - at + 64, c.dict_byte | OPEN)], mode)[0]
        assert not (alone[0] == 0 and alone[1] == c.plain[at:refs[0][2]]), c.name


def test_index_many_dictionary_resets():
    c = {c.name: c for c in B.directed_cases()}["dictionary-reset-0xE0-mid-stream-64-times"]
    run = len(c.plain) // 64                                              # 64 runs of as many bytes each, a reset in front of every one
    assert len(c.plain) == 64 * run and run % 16 != 0
    refs = units_of(c.stream, c.dict_byte)
    check_tiling(refs, c.stream, c.dict_byte)
    at = 0
    for _, _, uncomp, _ in refs[:-1]:                                     # cut only where the position is a multiple of 16, and at every such reset
        at += uncomp
        assert at % 16 == 0 and at % run == 0
    assert len(refs) == len([k for k in range(64) if k * run % 16 == 0]) >= 4


def test_index_of_a_stream_the_walk_cannot_follow():
    parts, z, refs = two_parts()
    n = refs[0][1]
    for bad in (z[:n] + b"\x55" + z[n:], z[:-40], z[:-1]):                # a wrong control byte; a chunk past the end; no end marker
        (off, comp, _, aux), = units_of(bad, DB)
        assert (off, comp, aux) == (0, len(bad), DB)
    lib = _lib.load()
    n_found = swc.C.c_size_t()
    assert lib.swc_index_blocks(8, b"", 0, None, 0, swc.C.byref(n_found)) == 0 and n_found.value == 1


# ------------------------------------------------------------------------------------------------------- units end to end
def decode_as_units(chunks, dict_byte, mode, want=None):
    """The units kind 8 lists through the emulation, under the acceptance rule.  Returns (number of units, accepted or None);
    where the units are not accepted the whole stream through the emulation equals the oracle."""
    refs = units_of(chunks, dict_byte)
    check_tiling(refs, chunks, dict_byte)
    res = R.run_jobs(chunks, [(off, comp, uncomp, aux) for off, comp, uncomp, aux in refs], mode)
    got = R.accept(refs, res) if len(refs) >= 2 else None
    if got is None:
        e = O.lzma2(bytes(chunks), dict_byte) if want is None else want
        cap = max(len(e[1]), 1) + (0 if e[0] == 0 else 300)
        (st, out, cons, out_len, aux), = R.run_jobs(chunks, [(0, len(chunks), cap, dict_byte)], mode)
        assert st == e[0] and aux == dict_byte
        if st == 0:
            assert (out, cons) == (e[1], e[2])
    return len(refs), got


@MODES
def test_directed_streams_as_units(mode):
    cases = [c for c in B.directed_cases() if c.kind == "lzma2" and c.status == 0]
    assert len(cases) >= 40
    most, cut = 0, 0
    for c in cases:
        n, got = decode_as_units(c.stream, c.dict_byte, mode, (0, c.plain, c.consumed))
        cut += n >= 2
        if got is not None:
            assert got == (c.plain, c.consumed), c.name
            most = max(most, n)
        if c.name == "match-reaching-behind-a-dictionary-reset":
            assert got is None
    assert most >= 3 and cut >= 1
    # the same construct with its reset where kind 8 cuts: the unit fails, the stream does not
    c = R.aligned_match_behind_reset()
    assert O.lzma2(c.stream, c.dict_byte) == (0, c.plain, c.consumed)
    refs = units_of(c.stream, c.dict_byte)
    assert [u for _, _, u, _ in refs] == [112, 32]
    n, got = decode_as_units(c.stream, c.dict_byte, mode, (0, c.plain, c.consumed))
    assert n == 2 and got is None
    res = R.run_jobs(c.stream, refs, mode)
    assert res[0][0] == 0 and res[0][4] & OPEN and res[1][0] != 0


@MODES
def test_random_streams_as_units(mode):
    rnd = random.Random(0x12A2B00)
    cases = []
    while len(cases) < 200:
        c = B.random_stream(rnd, rnd.choice([1, 9, 300, 4000, 20000]), len(cases) % 2 == 0)
        if c.kind == "lzma2":
            cases.append(c)
    accepted = 0
    for i, c in enumerate(cases):
        n, got = decode_as_units(c.stream, c.dict_byte, mode, (0, c.plain, c.consumed))
        if got is not None:
            assert got == (c.plain, c.consumed), "stream %d" % i
            accepted += 1
    assert accepted >= 5


@functools.lru_cache(maxsize=None)
def recipe_cases():
    """Recipe streams under four model shapes, their parts at aligned and odd positions, tiny stored parts among them."""
    rnd = random.Random(0x12A2C00)
    out = []
    for k, shape in enumerate(R.SHAPES * 3):
        sizes = [[4096, 4112, 33, 1000], [16, 1, 15, 160, 7, 9, 4000], [65536, 48, 3000, 5]][k % 3]
        parts = [R.text(n, 100 * k + i) if n > 20 else bytes(rnd.randrange(256) for _ in range(n)) for i, n in enumerate(sizes)]
        out.append((shape, parts, R.recipe(parts, shape)))
    return out


@MODES
def test_recipe_streams_as_units(mode):
    firsts = set()
    for shape, parts, z in recipe_cases():
        plain = b"".join(parts)
        want = O.lzma2(z, DB)
        assert want == (0, plain, len(z)), shape
        firsts |= {z[off] for off, *_ in units_of(z, DB)}
        n, got = decode_as_units(z, DB, mode, want)
        assert n >= 3 and got == (plain, len(z)), shape
    assert 0x01 in firsts and any(f >= 0xE0 for f in firsts)


def test_stand_alone_program_with_sanitizers(tmp_path):
    c = {c.name: c for c in B.directed_cases()}["dictionary-reset-0xE0-mid-stream-64-times"]
    _, parts, z = recipe_cases()[1]
    cases = [(c.stream, units_of(c.stream, c.dict_byte), c.consumed, c.plain), (z, units_of(z, DB), len(z), b"".join(parts))]
    assert all(len(refs) >= 3 for _, refs, _, _ in cases)
    # (unoptimised: the program holds the whole emulation library, and its two cases take no time to run)
    out = _emu.run_program(tmp_path, "emu_lzma2_runs.cpp", "EMU_LZMA2_RUNS_MAIN", R.case_file(cases), opt=("-O0",) + _emu.SANITIZED[1:])
    assert "2 cases, 0 mismatches" in out
