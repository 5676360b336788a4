"""CPU tier of the placement tests: the case lists of tests/_placement_cases.py through the host build of the device code with the
INPUTS at every residue mod 16 as well (tests/_emu.py: run_batch in_misalign; guard bytes around inputs and outputs, inputs checked
unchanged) -- what test_gpu_placement.py does on the device, where the kernels are the compiled ones.

Every input residue meets the output residues 0, 5 and 15; the payloads marked hot meet the full 16 x 16 cross (BZip2: the stream
blocks up to 4,000 bytes; the larger ones meet every input residue and three output residues).  The SIMT regions run in lane order 0
(forward) and 2 (shuffled): Deflate and LZ4 at every placement under both, the rest alternating from placement to placement so that
either order meets every input residue (the large BZip2 blocks: the two orders together).  Left to the device tier: the adjacent LZ4 prefix (run_batch places no
prefix in front of an output; tests/_emu_lz4_linked.py drives that path with its own buffers), and the checksums
(tests/test_checksum_emulation.py places their data already)."""
import pytest

import _emu as E
import _emu_dynamic as ED
import _placement_cases as P

PAIRS = [(i, o) for i in range(16) for o in (0, 5, 15)]
CROSS = [(i, o) for i in range(16) for o in range(16)]


def _order(i, o):
    return 0 if (i + o) % 2 == 0 else 2


def _sweep(pairs, run, cases, label, both=False, every_order_everywhere=True):
    """run(i, o) -> results of `cases` with the inputs at residue i and the outputs at residue o; compared with the expectations.
    both: every placement under lane order 0 and under 2, else under _order(i, o)."""
    seen_in, seen_out, orders = set(), set(), {}
    try:
        for i, o, order in [(i, o, k) for i, o in pairs for k in ((0, 2) if both else (_order(i, o),))]:
            E.set_order(order)
            orders.setdefault(order, set()).add(i)
            res = run(i, o)
            seen_in.add(i)
            seen_out.add(o)
            for c, r in zip(cases, res):
                what = "%s, %s, in %% 16 = %d, out %% 16 = %d, lane order %d" % (label, c.name, i, o, order)
                assert r[0] == c.status, "status %d, expected %d: %s" % (r[0], c.status, what)
                if c.out_len is not None:
                    assert r[3] == c.out_len, "out_len %d, expected %d: %s" % (r[3], c.out_len, what)
                if c.in_consumed is not None:
                    assert r[2] == c.in_consumed, "in_consumed %d, expected %d: %s" % (r[2], c.in_consumed, what)
                if c.status in (0, 901) and c.data is not None:
                    assert r[1] == c.data[:min(c.out_len, c.cap)], "bytes differ: " + what
    finally:
        E.set_order(0)
    assert seen_in == set(range(16)) and seen_out >= {0, 5, 15}
    assert orders[0] | orders[2] == set(range(16)) and (not every_order_everywhere or orders[0] == orders[2])
    return seen_out


@pytest.fixture(params=[1, 0], ids=["wave-copier", "workgroup-resolver"])
def copier(request):
    """Phase 2 of Deflate and LZ4 by lz_copy.h (what the emulation runs by default) and by lz_resolve.h."""
    E.lib.emu_set_copier(request.param)
    yield request.param
    E.lib.emu_set_copier(1)


def _inflate(cases):
    return lambda i, o: E.inflate([c.unit for c in cases], [c.cap for c in cases], misalign=o, in_misalign=i)


def test_deflate_at_every_input_residue(copier):
    _sweep(PAIRS, _inflate(P.DEFLATE), P.DEFLATE, "inflate, copier %d" % copier, both=True)


def test_deflate_hot_payloads_full_cross(copier):
    hot = [c for c in P.DEFLATE if c.hot]
    assert [c.name for c in hot] == ["text-5000", "mix-70001", "stored-7001"]
    assert _sweep(CROSS, _inflate(hot), hot, "inflate, copier %d" % copier, both=True) == set(range(16))


def _lz4(cases):
    return lambda i, o: E.lz4_block([c.unit for c in cases], [c.cap for c in cases], dicts=[c.dictionary for c in cases], misalign=o, in_misalign=i,
                                    aux=[c.aux for c in cases])


def test_lz4_blocks_at_every_input_residue(copier):
    cases = [c for c in P.LZ4 if not c.prefix]
    assert len(cases) == len(P.LZ4) - 1 and any(c.aux == P.LZ4_STORED for c in cases)
    _sweep(PAIRS, _lz4(cases), cases, "lz4_block, copier %d" % copier, both=True)


def test_lz4_hot_payloads_full_cross(copier):
    hot = [c for c in P.LZ4 if c.hot]
    assert len(hot) == 5
    assert _sweep(CROSS, _lz4(hot), hot, "lz4_block, copier %d" % copier, both=True) == set(range(16))


@pytest.mark.parametrize("mode", [1, 0], ids=["coder-cache", "coders-in-lds"])
def test_lzma2_and_lzma_at_every_input_residue(mode):
    two = [c for c in P.LZMA if c.codec == "lzma2"]
    one = [c for c in P.LZMA if c.codec == "lzma"]
    assert len(two) + len(one) == len(P.LZMA) and one
    _sweep(PAIRS, lambda i, o: E.lzma2([c.unit for c in two], [c.cap for c in two], [c.aux for c in two], mode=mode, misalign=o, in_misalign=i),
           two, "lzma2")
    _sweep(PAIRS, lambda i, o: E.lzma([c.unit for c in one], [c.cap for c in one], [c.lzma[:3] for c in one], [c.lzma[3] for c in one],
                                      [c.lzma[4] for c in one], mode=mode, misalign=o, in_misalign=i), one, "lzma")


def _bzip2(cases):
    return lambda i, o: E.bzip2_block([c.unit for c in cases], [c.extra for c in cases], [c.dict_value for c in cases],
                                      [c.cap for c in cases], lcap=140000, misalign=o, in_misalign=i)


@pytest.fixture(params=[None, (0, 0)], ids=["fused", "team"])
def team(request):
    E.set_bzip2_team(request.param)
    yield request.param
    E.set_bzip2_team(None)


def test_bzip2_small_blocks_full_cross(team):
    """The stream blocks of up to 4,000 bytes, the two built blocks and the wrong CRC at all 256 residue pairs -- the lay-out and the
    RLE1 undo at every output residue; the lane order alternates, and either order meets every residue of both sides."""
    small = [c for c in P.BZIP2 if c.cap <= 7949]
    assert len(small) == 9 and sum(c.hot for c in small) == 6
    assert _sweep(CROSS, _bzip2(small), small, "bzip2_block") == set(range(16))


def test_bzip2_large_blocks_at_every_input_residue(team):
    """The blocks of 50,000 to 100,000 bytes (nine tenths of this file's time were they crossed): every input residue -- all four
    residues mod 4 for each start bit the streams offer -- and the output residues 0, 5 and 15 in turn."""
    large = [c for c in P.BZIP2 if c.cap > 7949]
    assert len(large) == 8 and all(c.hot for c in large) and len({c.extra % 8 for c in large}) >= 3
    pairs = [(i, (0, 5, 15)[i % 3]) for i in range(16)]
    _sweep(pairs, _bzip2(large), large, "bzip2_block", every_order_everywhere=False)


def test_delta_at_every_residue_pair():
    for c in P.DELTA:
        assert E.delta_placed(c.unit, c.aux, c.at[0], c.at[1]) == c.data, (c.name, c.at)
    assert {c.at for c in P.DELTA} == {(i, o) for i in range(16) for o in range(16)}
    for c in P.DELTA_IN_PLACE:
        assert E.delta_placed(c.unit, c.aux, c.at[0], c.at[1], in_place=True) == c.data, (c.name, c.at)
    assert {c.at[1] for c in P.DELTA_IN_PLACE} == set(range(16))


@pytest.mark.parametrize("codec", ["lz4_compress", "deflate_compress", "deflate_compress_dynamic"])
def test_encoders_at_every_input_residue(codec):
    """Status 0 at the header's exact bound, bytes that decode to the input under the oracle and equal those at (0, 0).  Outputs of
    the Deflate encoders at the residues the header allows: 0, 4, 8, 12."""
    cases = P.ENCODERS[codec]
    outs = (0, 5, 15) if codec == "lz4_compress" else (0, 4, 8, 12)
    run = {"lz4_compress": lambda i, o: E.lz4_compress([c.source[1] for c in cases], [c.source[0] for c in cases], [c.cap for c in cases], misalign=o, in_misalign=i),
           "deflate_compress": lambda i, o: E.deflate_compress([c.unit for c in cases], [c.cap for c in cases], misalign=o, in_misalign=i),
           "deflate_compress_dynamic": lambda i, o: ED.deflate_compress_dynamic([c.unit for c in cases], [c.cap for c in cases], misalign=o, in_misalign=i)}[codec]
    try:
        E.set_order(0)
        base = run(0, 0)
        for c, r in zip(cases, base):
            assert r[0] == 0 and r[3] <= c.cap, (c.name, r[0], r[3])
            P.check_encoded(codec, c, r[1])
        seen = set()
        for i in range(16):
            for k, o in enumerate(outs):
                E.set_order(0 if (i + k) % 2 == 0 else 2)
                for c, r, b in zip(cases, run(i, o), base):
                    assert (r[0], r[1]) == (0, b[1]), "%s at in %% 16 = %d, out %% 16 = %d: not the bytes of (0, 0)" % (c.name, i, o)
                    if c.in_consumed is not None:
                        assert r[2] == c.in_consumed, c.name
                seen.add(i)
        assert seen == set(range(16))
    finally:
        E.set_order(0)
