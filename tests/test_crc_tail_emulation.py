"""CPU tier: the CRC tail of the Deflate copy kernel (csrc/crc32_tail.h) run on the host, its constants in exactly 6,144 bytes,
against zlib.crc32 -- every length at which the code takes another path, every start residue, every lane order."""
import zlib

import pytest

import _emu_crc_tail as T
from swcompression_amd import corpus

# rows of 2 KB, two rows per step (an odd row first), a ring of four rows: one byte either side of each of them, of an odd and an
# even number of rows behind a full ring, and of several turns of the ring
ROW = 2048
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33]
for size in (ROW, 2 * ROW, 3 * ROW, 4 * ROW, 5 * ROW, 8 * ROW, 12 * ROW, 13 * ROW, 16 * ROW):
    LENGTHS += [size - 1, size, size + 1]
LENGTHS += [65535, 65536, 65537, 1048575]
MAXLEN = max(LENGTHS)

DATA = {
    "text": corpus.p_text(MAXLEN, 41),
    "mix": corpus.p_mix(MAXLEN, 42),
    "zero": bytes(MAXLEN),
    "ones": b"\xff" * MAXLEN,
}
WANT = {(k, n): zlib.crc32(v[:n]) & 0xFFFFFFFF for k, v in DATA.items() for n in LENGTHS}


@pytest.fixture(autouse=True)
def _forward_again():
    yield
    T.set_order(0)


@pytest.mark.parametrize("order", [0, 1, 2], ids=["forward", "reverse", "shuffled"])
@pytest.mark.parametrize("kind", sorted(DATA))
def test_tail_matches_zlib(kind, order):
    T.set_order(order)
    data = DATA[kind]
    try:
        for n in LENGTHS:
            for residue in range(16):
                got = T.crc32(data[:n], residue)
                assert got == WANT[kind, n], "%s, %d bytes at residue %d, order %d: %08x, zlib %08x" % (kind, n, residue, order, got, WANT[kind, n])
    finally:
        T.set_order(0)
