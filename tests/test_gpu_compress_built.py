"""The four encoders on inputs BUILT against their parse (tests/_compress_cases.py), GPU tier.

LZ4, Deflate static and Deflate dynamic: all cases of a codec and its capacity jobs in ONE launch through the placement harness
(tests/_placed.py: guard bytes, verify()), every job's bytes those of the host emulation for the same case -- whose output the CPU
tier (tests/test_compress_built_emulation.py) holds to the oracle, to zlib / liblz4 and to the case's expectation.  The ten largest
cases once more through the single-shot calls.  BZip2.compress on every bzip2 case, byte for byte the emulation's stream: the
emulation sorts with std::stable_sort, the device with the three rocPRIM calls behind the prefix-doubling sort, and the tie-heavy
inputs here are where that part is held to account."""
import bz2
import collections
import zlib

import pytest

import _compress_cases as K
import _oracle as O
import test_compress_built_emulation as T
from _placed import PlacedBatch

pytestmark = pytest.mark.gpu

Expected = collections.namedtuple("Expected", "status out_len in_consumed data")
CODEC_NAMES = {"lz4": "lz4_compress", "static": "deflate_compress", "dynamic": "deflate_compress_dynamic"}


def _bound(kind, c):
    n = len(c.data)
    return n + n // 255 + 16 if kind == "lz4" else n + n // 8 + 32


@pytest.mark.parametrize("kind", ["lz4", "static", "dynamic"])
def test_all_cases_in_one_launch(kind):
    cases = T.CODECS[kind][0]
    emu = T.results(kind)
    full = dict(zip((c.name for c in cases), (r[1] for r in emu)))
    jobs = [(c, _bound(kind, c), Expected(r[0], r[3], r[2], r[1])) for c, r in zip(cases, emu)]
    for c, cap, status, size in T.capacity_jobs(kind):
        # below its capacity the dynamic path writes nothing (its sizes are known before the second pass): no bytes to compare
        data = full[c.name][:cap] if status == 0 or kind != "dynamic" else None
        jobs.append((c, cap, Expected(status, size, len(c.prefix if kind == "lz4" else b"") + len(c.data), data)))
    assert all(e.status == 0 for _, _, e in jobs[:len(cases)])
    lz4 = kind == "lz4"
    b = PlacedBatch(CODEC_NAMES[kind], [(c.prefix if lz4 else b"") + c.data for c, _, _ in jobs], [cap for _, cap, _ in jobs],
                    [i % 16 for i in range(len(jobs))], [(3 * i) % 16 if lz4 else 4 * (i % 4) for i in range(len(jobs))],
                    extra=[len(c.prefix) for c, _, _ in jobs] if lz4 else None)
    b.launch()
    b.verify([e for _, _, e in jobs])
    for i, (c, cap, e) in enumerate(jobs):
        if e.data is not None:
            assert b.produced(i) == e.data, "%s (out_cap %d): not the emulation's bytes" % (c.name, cap)
    assert sum(1 for _, _, e in jobs if e.status == 901) >= 12


def _largest(cases, count=10):
    return sorted(cases, key=lambda c: -len(c.data))[:count]


def test_single_shot_calls_on_the_largest_cases():
    import swcompression_amd as swc
    O.lib.refcpu_set_max_output(1 << 22)
    try:
        for c in _largest(K.DEFLATE + K.DYNAMIC):
            for dynamic in (False, True):
                z = swc.Deflate.compress(c.data, dynamic=dynamic)
                assert O.deflate(z) == (0, c.data, len(z)), (c.name, dynamic)
                assert zlib.decompress(z, -15) == c.data and swc.Deflate.decompress(z) == c.data, (c.name, dynamic)
                c.expect(K.deflate_tokens(z), "dynamic" if dynamic else "static")
        for c in _largest(K.LZ4):
            x = c.prefix + c.data                     # (the prefix in front, as the same buffer: dependent blocks reach into it)
            for block_size in (65536, 70000):
                f = swc.LZ4.compress(x, block_size=block_size, independent_blocks=False)
                assert O.lz4(f)[:2] == (0, x), (c.name, block_size)
                assert swc.LZ4.decompress(f) == x, (c.name, block_size)
    finally:
        O.lib.refcpu_set_max_output(1 << 30)


def test_bzip2_streams_are_the_emulations():
    import swcompression_amd as swc
    for c, (st, want) in zip(K.BZIP2, T.bzip2_results()):
        assert st == 0
        z = swc.BZip2.compress(c.data, block_size=c.prefix)         # (`prefix` of a bzip2 case: its level)
        assert z == want, "%s: the device's stream differs from the emulated stages'" % c.name
        assert swc.BZip2.decompress(z) == c.data, c.name
        assert bz2.decompress(z) == c.data, c.name
