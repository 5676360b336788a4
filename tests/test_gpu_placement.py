"""GPU tier: every codec with its inputs and outputs at all 16 residues mod 16, between guard bytes (tests/_placed.py), on the cases
of tests/_placement_cases.py, whose expectations are the oracle's.  include/swc_hip.h states one alignment rule for the pointers of
a job (`out` of the Deflate encoders is 4-byte aligned); every other placement is in contract, and the shipped kernels branch on
absolute addresses -- the bzip2 symbol loop in assembly refills from (in + next) & -4, the LZ4 copier fetches literal runs from the
block where it lies, the stage loads are 8 and 16 bytes wide at in + (ip & ~3), the copiers and the CRC-32 rows align by `out`.

One PlacedBatch of a few hundred to two thousand jobs per launch; verify() compares the whole output buffer with an image built on the host, the
inputs, the workspace guards and the IN fields of the records.  Every test runs with the fill 0xA5 and with 0x5A, so that a stray
write of the fill value itself cannot pass."""
import contextlib

import pytest

import _oracle as O
import _placement_cases as P
from _placed import PlacedBatch

pytestmark = pytest.mark.gpu

FILLS = [0xA5, 0x5A]
ALL = set(range(16))
SUMS = {"crc32": O.crc32, "adler32": O.adler32, "crc64": O.crc64, "bzip2crc32": O.bzip2crc32, "xxh32": O.xxh32}
_sum_cache = {}


DEFAULTS = {"lz_copier": 1, "deflate_team": 1, "lzma_coder_cache": 1, "bzip2_hot_cxx": 0, "bzip2_team_walk": 1}   # (include/swc_hip.h; the library has no getter)


@contextlib.contextmanager
def tuning(**values):
    """swc_set_tuning for the body; every key goes back to the library's default afterwards, whatever happened in between."""
    from swcompression_amd import _lib
    lib = _lib.load()
    try:
        for key, v in values.items():
            assert lib.swc_set_tuning(key.encode(), v) == 0, key
        yield
    finally:
        for key in values:
            lib.swc_set_tuning(key.encode(), DEFAULTS[key])


def _batch(codec, cases, places, fill):
    sel = [cases[k] for k, _, _ in places]
    return PlacedBatch(codec, [c.unit for c in sel], [c.cap for c in sel], [p[1] for p in places], [p[2] for p in places],
                       aux=[c.aux for c in sel], extra=[c.extra for c in sel] if any(c.extra for c in sel) else None,
                       dict_values=[c.dict_value for c in sel] if any(c.dict_value for c in sel) else None,
                       dicts=[c.dictionary for c in sel], prefixes=[c.prefix for c in sel], in_place=[c.in_place for c in sel],
                       same=[p[0] for p in places], fill=fill), sel


def _check_sums(b, sel, group):
    """swc_batch_checksum for all five kinds and swc_batch_crc32 over the outputs where they lie: [out, out + min(out_len, out_cap))
    of every job that produced bytes."""
    for kind in list(SUMS) + ["swc_batch_crc32"]:
        got = b.crc32() if kind == "swc_batch_crc32" else b.checksum(kind)
        fn = SUMS["crc32" if kind == "swc_batch_crc32" else kind]
        for i, c in enumerate(sel):
            if c.status in (0, 901):
                key = (kind, group, c.name)
                if key not in _sum_cache:
                    _sum_cache[key] = fn(c.data[:min(c.out_len, c.cap)])
                assert int(got[i]) == _sum_cache[key], "%s of %s at %s" % (kind, c.name, b.where(i))


@pytest.mark.parametrize("team", [1, 0, -1], ids=["team-auto", "one-wave", "team-forced"])
@pytest.mark.parametrize("copier", [1, -1], ids=["copier-auto", "wave-copier"])
@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_deflate(fill, copier, team):
    """Two launches.  822 streams: phase 1 by one wavefront per stream under "deflate_team" 1 and 0 (a team is the library's choice up
    to 256 streams), by the team of six wavefronts under -1 (inflate_sync.h / inflate_team.hip).  66 streams (every case at four
    residue pairs, no cross): the team under 1 -- the library's own choice -- and -1, one wavefront under 0.  Phase 2 in both:
    "lz_copier" 1 takes the workgroup resolver (lz_resolve.h; the wave copier starts at 2,560 streams), -1 forces the wave copier
    (lz_copy.h).  Then every checksum kernel over the outputs at their residues (two of them 700,001 bytes of 0xFF and of zeros:
    Adler-32's extremes), and the large batch once more through swc_batch_decompress_crc32_ws."""
    with tuning(lz_copier=copier, deflate_team=team):
        cases = P.DEFLATE + P.ADLER
        for places in (P.placements(cases, 0xDEF), P.placements(cases, 0xDE0, hot=False)):
            assert len(places) in (822, 66)
            b, sel = _batch("deflate", cases, places, fill)
            assert b.residues_launched() == (ALL, ALL)
            b.launch()
            b.verify(sel)
            _check_sums(b, sel, "deflate")
        b, sel = _batch("deflate", cases, P.placements(cases, 0xDEF), fill)
        b.launch(crc=True)
        b.verify(sel)
        got = b.fused_crc32()
        for i, c in enumerate(sel):
            if c.status in (0, 901):
                assert int(got[i]) == _sum_cache[("crc32", "deflate", c.name)], "fused CRC-32 of %s at %s" % (c.name, b.where(i))


@pytest.mark.parametrize("copier", [1, -1], ids=["copier-auto", "wave-copier"])
@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_lz4_blocks(fill, copier):
    """1,320 blocks per launch, with the workspace: the stripe parser (lz4_wave.h), then "lz_copier" 1 -> the workgroup resolver
    (lz_resolve.h; below 2,560 streams), -1 -> the wave copier (lz_copy.h: literal runs fetched from the block at its residue).  The
    prefix somewhere else goes to the lane decoder (lz4_lane.h), the adjacent prefix and SWC_LZ4_STORED to the chain copier."""
    with tuning(lz_copier=copier):
        places = P.placements(P.LZ4, 0x124)
        b, sel = _batch("lz4_block", P.LZ4, places, fill)
        assert b.residues_launched() == (ALL, ALL)
        b.launch()
        b.verify(sel)
        _check_sums(b, sel, "lz4")


@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_lz4_blocks_lane_decoder_without_workspace(fill):
    """swc_batch_decompress without a workspace: every block by the one-block-per-lane kernel (lz4_lane.h).  Without SWC_LZ4_STORED,
    which needs the workspace."""
    cases = [c for c in P.LZ4 if not c.aux]
    assert len(cases) == len(P.LZ4) - 1
    b, sel = _batch("lz4_block", cases, P.placements(cases, 0x125), fill)
    assert b.residues_launched() == (ALL, ALL)
    b.launch(workspace=False)
    b.verify(sel)


@pytest.mark.parametrize("cache", [1, 0], ids=["coder-cache", "coders-in-lds"])
@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_lzma2_and_lzma(fill, cache):
    """Every case at 16 residue pairs, one launch per codec; "lzma_coder_cache" 1: LDS as a cache of the literal coders in the
    workspace, 0: the coders of lc + lp <= 3 in LDS (lzma_wave.h)."""
    with tuning(lzma_coder_cache=cache):
        seen = (set(), set())
        for codec in ("lzma2", "lzma"):
            cases = [c for c in P.LZMA if c.codec == codec]
            b, sel = _batch(codec, cases, P.placements(cases, 0x17A, per_case=16), fill)
            for s, r in zip(seen, b.residues_launched()):
                s |= r
            b.launch()
            b.verify(sel)
        assert seen == (ALL, ALL)


@pytest.mark.parametrize("walk", [1, 0, 2], ids=["walk-auto", "walk-fused", "walk-team"])
@pytest.mark.parametrize("cxx", [0, 1], ids=["isa", "cxx"])
@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_bzip2_blocks(fill, cxx, walk):
    """Every block of the level-1 streams at all 256 residue pairs -- all four (in + next) & -4 phases of the assembly refill for every
    start bit the streams offer, the lay-out and the RLE1 undo at every output residue -- as three launches: the blocks of the streams
    up to 79,999 bytes with the two built blocks and the wrong CRC (16 pairs each; 2,096 jobs), the three blocks of the 250,000 bytes
    of text, and those of mix (768 jobs each).  `aux` must come back as the CRC-32 of the block's output, in_consumed as the bit
    offset behind the block (include/swc_hip.h).  "bzip2_hot_cxx" 0: the symbol loop in assembly (hot_symbols_isa), 1: its C++
    twin; "bzip2_team_walk" 0: one wavefront takes a block through all stages (bzip2_block.h), 2: stage 3 as the team kernels
    (bzip2_team.h), 1: the library's choice, the team kernels for launches of this size."""
    with tuning(bzip2_hot_cxx=cxx, bzip2_team_walk=walk):
        groups = [[c for c in P.BZIP2 if "250000" not in c.name]] + [[c for c in P.BZIP2 if c.name.startswith(k + "-250000")] for k in ("text", "mix")]
        assert sum(len(g) for g in groups) == len(P.BZIP2) and [len(g) for g in groups[1:]] == [3, 3]
        offered = set()
        for cases in groups:
            places = P.placements(cases, 0xB22, per_case=16)
            b, sel = _batch("bzip2_block", cases, places, fill)
            assert b.residues_launched() == (ALL, ALL)
            for k, c in enumerate(cases):
                if c.hot:
                    assert {(p[1], p[2]) for p in places if p[0] == k} == {(i, o) for i in ALL for o in ALL}
                    offered.add(c.extra % 8)
            assert all(c.aux_out is not None for c in cases)
            b.launch()
            b.verify(sel)
        assert len(offered) >= 3


@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_delta(fill):
    """out != in at all 256 residue pairs, out == in at all 16 residues (delta_group.h)."""
    cases = P.DELTA + P.DELTA_IN_PLACE
    places = [(k, c.at[0], c.at[1]) for k, c in enumerate(cases)]
    b, sel = _batch("delta", cases, places, fill)
    assert {(p[1], p[2]) for p in places[:256]} == {(i, o) for i in ALL for o in ALL} and {p[2] for p in places[256:]} == ALL
    assert b.residues_launched() == (ALL, ALL)
    b.launch()
    b.verify(sel)


@pytest.mark.parametrize("codec", ["lz4_compress", "deflate_compress", "deflate_compress_dynamic"])
@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_encoders(fill, codec):
    """Inputs at all 16 residues, outputs at all 16 (LZ4) or at 0, 4, 8, 12 (the Deflate encoders: the header's rule), out_cap
    exactly the header's bound: status 0, bytes that decode to the input under the oracle's decoder, which consumes all of them, and
    that equal the bytes of the same unit at (0, 0) -- verify() holds jobs over one unit to the same bytes."""
    cases = P.ENCODERS[codec]
    deflate = codec != "lz4_compress"
    places = P.encoder_placements(cases, deflate)
    b, sel = _batch(codec, cases, places, fill)
    assert b.residues_launched() == (ALL, {0, 4, 8, 12} if deflate else ALL)
    b.launch()
    b.verify(sel)
    for i, (p, c) in enumerate(zip(places, sel)):
        assert int(b.res["out_len"][i]) <= c.cap, c.name
        if (p[1], p[2]) == (0, 0):
            P.check_encoded(codec, c, b.produced(i))


@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_the_harness_sees_what_it_is_for(fill):
    """verify() itself: after a clean launch, one byte changed behind a job's capacity, in front of its output, inside its bytes,
    in its input, on either side of the workspace, and in an IN field of its record -- each must fail, with the job named."""
    import numpy as np
    cases = P.DELTA[:48]
    b, sel = _batch("delta", cases, [(k, c.at[0], c.at[1]) for k, c in enumerate(cases)], fill)
    b.launch()
    b.verify(sel)
    k = next(i for i, c in enumerate(sel) if len(c.unit) == 5000)
    clean = b.out_got.copy()
    for off, what in ((b.caps[k], "behind"), (-1, "in front"), (-b.guard, "in front"), (b.caps[k] + b.guard - 1, "behind"), (17, "inside")):
        b.out_got = clean.copy()
        b.out_got[b.out_off[k] + off] ^= 0xFF
        with pytest.raises(AssertionError, match="output buffer differs"):
            b.verify(sel)
    b.out_got = clean.copy()
    b.d_in[b.in_off[k] + 100] ^= 0xFF
    with pytest.raises(AssertionError, match=r"input buffer changed.*job %d " % k):
        b.verify(sel)
    b.d_in[b.in_off[k] + 100] ^= 0xFF
    for at, word in ((4095, "in front of"), (4096 + b.ws_bytes, "behind")):
        b.d_ws[at] ^= 0xFF
        with pytest.raises(AssertionError, match="the launch wrote %s its workspace" % word):
            b.verify(sel)
        b.d_ws[at] ^= 0xFF
    for f in ("in", "in_len", "out", "out_cap", "dict", "dict_len", "aux"):
        keep = b.res.copy()
        b.res[f][k] += 1
        with pytest.raises(AssertionError, match="job %d .*(field|aux)" % k):
            b.verify(sel)
        b.res = keep
    b.res["status"][k] = 901
    with pytest.raises(AssertionError, match="status 901, expected 0"):
        b.verify(sel)
