"""GPU tier: a soak of the two LZ77 decode paths (Deflate, LZ4 block) and of LZMA2 / BZip2 on randomly BUILT streams, against the oracle; the three encoders on the same kind of text.

The other GPU tests take their streams from encoders, which never produce most of what the formats allow.  Here the LZ4
blocks are assembled sequence by sequence (LZ4.swift:341-412) from random literal-run lengths, match lengths and offsets
that sit on and around every boundary of the two kernels' record formats (literal runs of 14 / 15 / 16 / 269 / 270 and of
kilobytes, match lengths of 18 / 19 / 20 / 273 / 274 and of tens of kilobytes, offsets of 1 .. 65,535 including the ones that
reach exactly to the start of the output), and the Deflate streams come from zlib over plain text that is itself a random
splice of payload classes and copies of earlier stretches at every distance up to the window -- and, since zlib is a narrow
encoder too, from a builder of their own (_deflate_build.py) that writes them code by code.  Every stream is decoded by
the oracle; the engine must return the oracle's status and -- for status 0 -- its bytes, consumed input and length; damaged
copies (bit flips, truncations, garbage tails) must return the oracle's status.  Each round runs once with the library's
choice of phase-2 kernel and once with the wave kernel forced.

SWC_SOAK_ROUNDS (default 2) sets the number of seeded rounds; profiles/r06z_soak_gpu.log holds runs of 300 - 1,500 rounds per test.
"""
import os
import random

import pytest

import _deflate_build as B
import _lzma_build as LB
import _oracle as O
import _soak as K
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu

ROUNDS = int(os.environ.get("SWC_SOAK_ROUNDS", "2"))


def _both_kernels(fn):
    from swcompression_amd import _lib
    lib = _lib.load()
    try:
        for mode in (1, -1):
            assert lib.swc_set_tuning(b"lz_copier", mode) == 0
            fn("auto" if mode == 1 else "wave")
    finally:
        lib.swc_set_tuning(b"lz_copier", 1)


def _check(codec, streams, exp, caps, label, aux=None, extra=None, dict_values=None):
    b = DeviceBatch(codec, streams, caps, aux=aux, extra=extra, dict_values=dict_values)
    b.launch(sync=True)
    r = b.results()
    for i, e in enumerate(exp):
        what = "%s, stream %d (%d bytes in, oracle status %d)" % (label, i, len(streams[i]), e[0])
        assert int(r["status"][i]) == e[0], "status %d: %s" % (int(r["status"][i]), what)
        if e[0] == 0:
            assert int(r["out_len"][i]) == len(e[1]) and int(r["in_consumed"][i]) == e[2], what
            assert b.output(i, len(e[1])) == e[1], "bytes differ: " + what


@pytest.mark.parametrize("seed", range(ROUNDS))
def test_lz4_blocks_built_sequence_by_sequence(seed):
    rnd = random.Random(0x4C5A34 + seed)
    O.lib.refcpu_set_max_output(1 << 24)
    try:
        streams = []
        for i in range(220):
            z, p = K.random_lz4_block(rnd, rnd.choice([1, 40, 700, 5000, 66000, 140000, 600000, 2500000]))
            st, out = O.lz4_block(z)[:2]
            assert out == p[:len(out)] and (st != 0 or out == p), "the builder and the oracle disagree on a block it built (seed %d, block %d)" % (seed, i)
            streams.append(z)
        streams += [K.damage(rnd, streams[rnd.randrange(len(streams))]) for _ in range(160)]
        exp = [O.lz4_block(z) + (len(z),) for z in streams]   # (a block that decodes is consumed whole)
        keep = [i for i, e in enumerate(exp) if e[0] != 901]
        caps = [max(len(exp[i][1]), 1) + rnd.choice([0, 0, 0, 3, 64]) for i in keep]
        _both_kernels(lambda label: _check("lz4_block", [streams[i] for i in keep], [exp[i] for i in keep], caps, "seed %d, %s" % (seed, label)))
    finally:
        O.lib.refcpu_set_max_output(1 << 30)


@pytest.mark.parametrize("seed", range(ROUNDS))
def test_deflate_streams_over_spliced_text(seed):
    rnd = random.Random(0xDEF1A7E + seed)
    O.lib.refcpu_set_max_output(1 << 24)
    try:
        streams = []
        for i in range(260):
            z = K.random_deflate_stream(rnd, rnd.choice([0, 1, 9, 300, 4000, 65536, 70000, 200000, 700000]), 7000 * seed + i)
            streams.append(z)
        streams += [K.damage(rnd, streams[rnd.randrange(len(streams))]) for _ in range(200)]
        exp = [O.deflate(z) for z in streams]
        keep = [i for i, e in enumerate(exp) if e[0] != 901]
        caps = [max(len(exp[i][1]), 1) + rnd.choice([0, 0, 0, 5]) for i in keep]
        from swcompression_amd import _lib
        lib = _lib.load()
        try:
            for team in (1, 0, -1):   # phase 1: the library's choice (launches of up to 256 streams: a team of wavefronts per stream), one wavefront per stream, teams forced
                assert lib.swc_set_tuning(b"deflate_team", team) == 0
                _both_kernels(lambda label: _check("deflate", [streams[i] for i in keep], [exp[i] for i in keep], caps, "seed %d, team %d, %s" % (seed, team, label)))
        finally:
            lib.swc_set_tuning(b"deflate_team", 1)
    finally:
        O.lib.refcpu_set_max_output(1 << 30)


BUILT_SEED = 0xB111D0DE
BUILT_STREAMS, BUILT_DAMAGED = 120, 100


@pytest.mark.parametrize("seed", range(ROUNDS))
def test_deflate_streams_built_code_by_code(seed):
    """Streams no encoder writes (tests/_deflate_build.py: all three block types, random complete code sets up to 15 bits, header
    runs across the literal / distance boundary, every distance up to 32,768, 258 as 284 + 31, blocks of a few tokens) and damaged
    copies of them.  Built once per seed, then the three forms of phase 1 times both copy kernels."""
    rnd = random.Random(BUILT_SEED + seed)
    O.lib.refcpu_set_max_output(1 << 24)
    try:
        streams = []
        for i in range(BUILT_STREAMS):
            # (four streams of 200,000 bytes per seed, none of them in the tiny-block style: building in Python, not decoding, is what they cost)
            z, p, body = B.random_stream(rnd, 200000 if i < 4 else rnd.choice([0, 1, 9, 300, 4000, 65536, 70000]), (i + seed) % (3 if i < 4 else 4))
            assert O.deflate(z) == (0, p, body), "the builder and the oracle disagree on a stream it built (seed %d, stream %d)" % (seed, i)
            streams.append(z)
        streams += [K.damage(rnd, streams[rnd.randrange(BUILT_STREAMS)]) for _ in range(BUILT_DAMAGED)]
        exp = [O.deflate(z) for z in streams]
        keep = [i for i, e in enumerate(exp) if i < BUILT_STREAMS or e[0] != 901]   # (no undamaged stream is ever left out)
        assert len(streams) - len(keep) <= BUILT_DAMAGED // 10, "%d damaged copies beyond the oracle's output cap" % (len(streams) - len(keep))
        caps = [max(len(exp[i][1]), 1) + rnd.choice([0, 0, 0, 5]) for i in keep]
        from swcompression_amd import _lib
        lib = _lib.load()
        try:
            for team in (1, 0, -1):
                assert lib.swc_set_tuning(b"deflate_team", team) == 0
                _both_kernels(lambda label: _check("deflate", [streams[i] for i in keep], [exp[i] for i in keep], caps, "seed %d, team %d, %s" % (seed, team, label)))
        finally:
            lib.swc_set_tuning(b"deflate_team", 1)
    finally:
        O.lib.refcpu_set_max_output(1 << 30)


@pytest.mark.parametrize("seed", range(ROUNDS))
def test_lzma2_units_of_random_encoder_settings(seed):
    """The range decoder's decision is one block of gfx950 instructions (lzma_wave.h: bit()): every lc / lp / pb,
    dictionaries from 4 KiB, both layouts of the literal coders."""
    from swcompression_amd import _lib
    lib = _lib.load()
    rnd = random.Random(0x7A4C + seed)
    O.lib.refcpu_set_max_output(1 << 24)
    try:
        units = [K.random_lzma2_unit(rnd, rnd.choice([0, 1, 9, 300, 4000, 70000, 300000]), 5000 * seed + i) for i in range(96)]
        units += [(K.damage(rnd, z), db) for z, db in (units[rnd.randrange(len(units))] for _ in range(64))]
        exp = [O.lzma2(z, db) for z, db in units]
        keep = [i for i, e in enumerate(exp) if e[0] != 901]
        caps = [max(len(exp[i][1]), 1) + rnd.choice([0, 0, 64]) for i in keep]
        try:
            for mode in (1, 0):
                assert lib.swc_set_tuning(b"lzma_coder_cache", mode) == 0
                _check("lzma2", [units[i][0] for i in keep], [exp[i] for i in keep], caps, "seed %d, coder cache %d" % (seed, mode), aux=[units[i][1] for i in keep])
        finally:
            lib.swc_set_tuning(b"lzma_coder_cache", 1)
    finally:
        O.lib.refcpu_set_max_output(1 << 30)


@pytest.mark.parametrize("seed", range(ROUNDS))
def test_lzma_streams_built_decision_by_decision(seed):
    """Streams no encoder writes (tests/_lzma_build.py: every chunk control in any order, property changes and dictionary resets in
    mid-stream, lc + lp up to 12, matches across resets, end markers inside chunks, raw LZMA with dictionaries of a few bytes); half
    of them restricted to what liblzma decodes.  100 per seed, LZMA2 and raw LZMA each in one launch, both layouts of the model."""
    from swcompression_amd import _lib
    lib = _lib.load()
    rnd = random.Random(0x12A4B50AC + seed)
    cases = [LB.random_stream(rnd, rnd.choice([1, 9, 300, 4000, 20000]), i % 2 == 0) for i in range(100)]
    exp = [O.lzma2(c.stream, c.dict_byte) if c.kind == "lzma2" else O.lzma_raw(c.stream, *c.props) for c in cases]
    for i, (c, e) in enumerate(zip(cases, exp)):
        assert e == (0, c.plain, c.consumed), "the builder and the oracle disagree on a stream it built (seed %d, stream %d)" % (seed, i)
    l2 = [i for i, c in enumerate(cases) if c.kind == "lzma2"]
    l1 = [i for i, c in enumerate(cases) if c.kind == "lzma"]
    assert l1 and l2
    caps = [max(len(c.plain), 1) for c in cases]      # exact capacity
    try:
        for mode in (1, 0):
            assert lib.swc_set_tuning(b"lzma_coder_cache", mode) == 0
            label = "seed %d, coder cache %d" % (seed, mode)
            _check("lzma2", [cases[i].stream for i in l2], [exp[i] for i in l2], [caps[i] for i in l2], label + ", LZMA2", aux=[cases[i].dict_byte for i in l2])
            p = [cases[i].props for i in l1]
            _check("lzma", [cases[i].stream for i in l1], [exp[i] for i in l1], [caps[i] for i in l1], label + ", raw LZMA",
                   aux=[lc | lp << 8 | pb << 16 for lc, lp, pb, _, _ in p], extra=[q[4] & 0xFFFFFFFFFFFFFFFF for q in p], dict_values=[q[3] for q in p])
    finally:
        lib.swc_set_tuning(b"lzma_coder_cache", 1)


@pytest.mark.parametrize("seed", range(ROUNDS))
def test_bzip2_streams_over_spliced_text(seed):
    """libbz2 at every block size over spliced text (zero runs and distance-1 copies: runs of every length for the RLE1 undo, the
    ones of 4 .. 259 bytes and the megabyte ones), damaged copies; all archives of a round in one launch, the inverse BWT once as
    the team kernels and once inside the block's wavefront."""
    import bz2
    import swcompression_amd as swc
    from swcompression_amd import _lib
    lib = _lib.load()
    rnd = random.Random(0xB2 + 977 * seed)
    O.lib.refcpu_set_max_output(1 << 24)
    try:
        streams = [bz2.compress(K.spliced_plain(rnd, rnd.choice([0, 1, 9, 300, 4000, 70000, 250000, 1200000]), 3000 * seed + i), rnd.randrange(1, 10)) for i in range(48)]
        streams += [K.damage(rnd, streams[rnd.randrange(len(streams))]) for _ in range(48)]
        exp = [O.bzip2(z) for z in streams]
        keep = [i for i, e in enumerate(exp) if e[0] != 901]
        try:
            for mode in (2, 0):
                assert lib.swc_set_tuning(b"bzip2_team_walk", mode) == 0
                got = swc.unarchive_many("bzip2", [streams[i] for i in keep])
                for k, i in enumerate(keep):
                    what = "seed %d, team walk %d, stream %d (%d bytes in)" % (seed, mode, i, len(streams[i]))
                    assert got[k][0] == exp[i][0], "status %d, oracle %d: %s" % (got[k][0], exp[i][0], what)
                    if exp[i][0] == 0:
                        assert got[k][1] == exp[i][1], "bytes differ: " + what
        finally:
            lib.swc_set_tuning(b"bzip2_team_walk", 1)
    finally:
        O.lib.refcpu_set_max_output(1 << 30)


@pytest.mark.parametrize("seed", range(ROUNDS))
def test_encoders_on_spliced_text(seed):
    """The three encoders on spliced text of random sizes (Deflate.compress beyond the megabyte above which it works in segments,
    LZ4 frames of every block size with and without linked blocks, BZip2 at every block size): the ORACLE's decoder, which must
    consume the whole stream, and the system's codec return the input."""
    import bz2
    import zlib
    import swcompression_amd as swc
    rnd = random.Random(0xE2C + 31 * seed)
    O.lib.refcpu_set_max_output(1 << 24)
    try:
        for i in range(10):
            p = K.spliced_plain(rnd, rnd.choice([0, 1, 2, 3, 9, 300, 4000, 65536, 300000, 1048576, 1048577, 2500000]), 800 * seed + i)
            z = swc.Deflate.compress(p)
            assert O.deflate(z) == (0, p, len(z)), "Deflate.compress, seed %d, buffer %d (%d bytes)" % (seed, i, len(p))
            assert zlib.decompress(z, -15) == p
        for i in range(10):
            p = K.spliced_plain(rnd, rnd.choice([0, 1, 12, 13, 300, 4000, 65536, 65537, 300000, 2500000]), 900 * seed + i)
            kw = dict(independent_blocks=rnd.random() < 0.5, block_checksums=rnd.random() < 0.5, content_checksum=rnd.random() < 0.5,
                      content_size=rnd.random() < 0.5, block_size=rnd.choice([173, 1024, 65536, 65537, 200000, 1 << 20, 4 << 20]))
            z = swc.LZ4.compress(p, **kw)
            assert O.lz4(z) == (0, p, len(z)), "LZ4.compress, seed %d, buffer %d (%d bytes, %r)" % (seed, i, len(p), kw)
        for i in range(6):
            p = K.spliced_plain(rnd, rnd.choice([0, 1, 9, 300, 4000, 99999, 100000, 100001, 250000, 1000000]), 700 * seed + i)
            bs = rnd.randrange(1, 10)
            z = swc.BZip2.compress(p, bs)
            assert O.bzip2(z) == (0, p, len(z)), "BZip2.compress, seed %d, buffer %d (%d bytes, block size %d)" % (seed, i, len(p), bs)
            assert bz2.decompress(z) == p
    finally:
        O.lib.refcpu_set_max_output(1 << 30)
