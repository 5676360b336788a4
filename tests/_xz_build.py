"""An .xz stream composed block by block (the .xz file format 1.0.4; what XZArchive.swift:90-192 and XZBlock.swift:18-97 read): raw
LZMA2 data from liblzma behind block headers written here, the padding, a check of any of the four types, the index and the footer.
`xz --block-size` is not needed to get a stream of many blocks, and a test knows where every field lies.  TEST INFRASTRUCTURE ONLY."""
import hashlib
import lzma
import struct
import zlib

CHECK_NONE, CHECK_CRC32, CHECK_CRC64, CHECK_SHA256 = 0x00, 0x01, 0x04, 0x0A
CHECK_SIZE = {CHECK_NONE: 0, CHECK_CRC32: 4, CHECK_CRC64: 8, CHECK_SHA256: 32}
DICT_SIZE, DICT_BYTE = 1 << 20, 16   # (2 | (b & 1)) << (b / 2 + 11)

_CRC64_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0xC96C5795D7870F42 if _c & 1 else 0)
    _CRC64_TABLE.append(_c)


def crc64(data):
    """CRC-64 of the .xz format (ECMA-182, reflected)."""
    c = 0xFFFFFFFFFFFFFFFF
    for b in data:
        c = _CRC64_TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFFFFFFFFFF


def multibyte(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def check_field(check, data):
    if check == CHECK_CRC32:
        return struct.pack("<I", zlib.crc32(data) & 0xFFFFFFFF)
    if check == CHECK_CRC64:
        return struct.pack("<Q", crc64(data))
    if check == CHECK_SHA256:
        return hashlib.sha256(data).digest()
    return b""


def raw_lzma2(data, preset=1):
    return lzma.compress(bytes(data), format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": preset, "dict_size": DICT_SIZE}])


def _pad4(n):
    return bytes(-n % 4)


class Built:
    """.stream: the bytes; .blocks: per block a dict of offsets into the stream -- header, data, check -- and comp / uncomp sizes."""

    def __init__(self, stream, blocks):
        self.stream, self.blocks = stream, blocks

    def flipped(self, offset, bit=0):
        s = bytearray(self.stream)
        s[offset] ^= 1 << bit
        return bytes(s)

    def with_damaged_check(self, k, byte=0, bit=0):
        """The stream with one bit of block k's check field flipped."""
        assert self.blocks[k]["check_size"] > byte
        return self.flipped(self.blocks[k]["check"] + byte, bit)


def build(payloads, check=CHECK_SHA256, sizes_in_header=True, preset=1):
    """One stream with a block per payload, every block LZMA2 alone."""
    flags = bytes([0, check])
    out = bytearray(b"\xFD7zXZ\x00" + flags + struct.pack("<I", zlib.crc32(flags) & 0xFFFFFFFF))
    records, blocks = [], []
    for p in payloads:
        p = bytes(p)
        comp = raw_lzma2(p, preset)
        body = bytes([0xC0 if sizes_in_header else 0x00])
        if sizes_in_header:
            body += multibyte(len(comp)) + multibyte(len(p))
        body += multibyte(0x21) + multibyte(1) + bytes([DICT_BYTE])
        body += _pad4(1 + len(body))
        header = bytes([(1 + len(body) + 4) // 4 - 1]) + body
        header += struct.pack("<I", zlib.crc32(header) & 0xFFFFFFFF)
        at = len(out)
        out += header + comp + _pad4(len(comp))
        field = check_field(check, p)
        blocks.append({"header": at, "data": at + len(header), "comp": len(comp), "uncomp": len(p), "check": len(out), "check_size": len(field)})
        out += field
        records.append((len(header) + len(comp) + len(field), len(p)))
    index = b"\x00" + multibyte(len(records)) + b"".join(multibyte(a) + multibyte(b) for a, b in records)
    index += _pad4(len(index))
    index += struct.pack("<I", zlib.crc32(index) & 0xFFFFFFFF)
    out += index
    tail = struct.pack("<I", len(index) // 4 - 1) + flags
    out += struct.pack("<I", zlib.crc32(tail) & 0xFFFFFFFF) + tail + b"YZ"
    return Built(bytes(out), blocks)


def cut(payload, block):
    """`payload` in pieces of `block` bytes, the last one short (or none for an empty payload)."""
    return [payload[i:i + block] for i in range(0, len(payload), block)]
