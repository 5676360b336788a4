"""Self-check of tests/_xz_build.py: the streams it composes are .xz streams to liblzma and to the oracle, with every check type,
with and without the size fields, from no block to many; a damaged check field is the reference's wrongCheck, carrying the data."""
import lzma

import pytest

import _oracle as O
import _xz_build as X
from swcompression_amd import corpus

WRONG_CHECK = 807
CHECKS = [X.CHECK_NONE, X.CHECK_CRC32, X.CHECK_CRC64, X.CHECK_SHA256]


def test_crc64_known_answer():
    assert X.crc64(b"123456789") == 0x995DC9BBDF1939FA


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("sizes", [True, False])
def test_built_streams_decode(check, sizes):
    payload = corpus.p_text(9000, 3) + corpus.p_rand(700, 4) + corpus.p_mix(5000, 5)
    for pieces in ([], [b""], [payload], X.cut(payload, 4096), X.cut(payload, 1000) + [b"", b"x"]):
        b = X.build(pieces, check, sizes_in_header=sizes)
        want = b"".join(pieces)
        assert lzma.decompress(b.stream, format=lzma.FORMAT_XZ) == want
        assert O.xz_unarchive(b.stream) == (0, want)
        assert len(b.blocks) == len(pieces)
        for blk, p in zip(b.blocks, pieces):
            assert b.stream[blk["check"]:blk["check"] + blk["check_size"]] == X.check_field(check, p)
            assert lzma.decompress(b.stream[blk["data"]:blk["data"] + blk["comp"]], format=lzma.FORMAT_RAW,
                                   filters=[{"id": lzma.FILTER_LZMA2, "dict_size": X.DICT_SIZE}]) == p


@pytest.mark.parametrize("check", CHECKS[1:])
def test_damaged_check_is_wrong_check_with_the_data(check):
    payload = corpus.p_text(20000, 9)
    pieces = X.cut(payload, 4096)
    b = X.build(pieces, check)
    for k in (0, 2, len(pieces) - 1):
        bad = b.with_damaged_check(k, byte=X.CHECK_SIZE[check] - 1, bit=5)
        st, data = O.xz_unarchive(bad)
        assert st == WRONG_CHECK
        assert data == b"".join(pieces[:k + 1])   # XZArchive.swift:44: the error carries the result so far, the failing block included
        with pytest.raises(lzma.LZMAError):
            lzma.decompress(bad, format=lzma.FORMAT_XZ)
