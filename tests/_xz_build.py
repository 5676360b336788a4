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


_ABSENT = object()


def _integer(v):
    """A multibyte integer, or bytes written as they are (an encoding that multibyte() would not produce)."""
    return bytes(v) if isinstance(v, (bytes, bytearray)) else multibyte(v)


def block(payload=b"", **fields):
    """One block of stream(): the payload and the fields to write differently (see stream())."""
    return dict(fields, payload=bytes(payload))


def stream(blocks=(), check=CHECK_CRC32, magic=b"\xFD7zXZ\x00", flags=None, header_crc=None, indicator=0, count=None, records=None,
           index_padding=None, index_crc=None, footer_crc=None, backward=None, footer_flags=None, footer_magic=b"YZ", padding=b""):
    """One stream with every field of the format an argument; None = the valid value.  An integer may be given as bytes, which are
    written as they are.
    Stream header: magic, flags (two bytes), header_crc.
    blocks: dicts from block(): comp (the LZMA2 data, None = liblzma's of the payload with DICT_SIZE), size_byte (the header size byte),
    flags (the block flags byte, None = filters - 1 and the bits of the sizes present), comp_size / uncomp_size (True = present and
    right, None = absent, else the value), filters ([(id, property bytes)] or [(id, property bytes, property size)]; the default is
    LZMA2 with dict_byte, default DICT_BYTE), header_padding (bytes), header_crc, block_padding (bytes), check_field (bytes).
    Index: indicator, count, records ([(unpadded size, uncompressed size)]), index_padding (bytes), index_crc.
    Footer: footer_crc, backward (the stored word), footer_flags (two bytes), footer_magic.  padding: bytes behind the stream."""
    flags = bytes([0, check]) if flags is None else bytes(flags)
    out = bytearray(magic + flags + struct.pack("<I", zlib.crc32(flags) & 0xFFFFFFFF if header_crc is None else header_crc))
    real, layout = [], []
    check_size = CHECK_SIZE.get(check, 0)
    for b in blocks:
        p = b["payload"]
        comp = b.get("comp")
        if comp is None:
            comp = raw_lzma2(p)
        filters = b.get("filters")
        if filters is None:
            filters = [(0x21, bytes([b.get("dict_byte", DICT_BYTE)]))]
        cs, us = b.get("comp_size", True), b.get("uncomp_size", True)
        bf = b.get("flags")
        if bf is None:
            bf = (len(filters) - 1) | (0x40 if cs is not None else 0) | (0x80 if us is not None else 0)
        body = bytes([bf])
        if cs is not None:
            body += _integer(len(comp) if cs is True else cs)
        if us is not None:
            body += _integer(len(p) if us is True else us)
        for f in filters:
            body += _integer(f[0]) + _integer(f[2] if len(f) > 2 else len(f[1])) + bytes(f[1])
        hp = b.get("header_padding")
        body += _pad4(1 + len(body)) if hp is None else bytes(hp)
        sb = b.get("size_byte")
        header = bytes([((1 + len(body) + 4) // 4 - 1) & 0xFF if sb is None else sb]) + body
        hc = b.get("header_crc")
        header += struct.pack("<I", zlib.crc32(header) & 0xFFFFFFFF if hc is None else hc)
        at = len(out)
        bp = b.get("block_padding")
        out += header + comp + (_pad4(len(header) + len(comp)) if bp is None else bytes(bp))
        field = b.get("check_field")
        if field is None:
            field = check_field(check, p)
        layout.append({"header": at, "data": at + len(header), "comp": len(comp), "uncomp": len(p), "check": len(out), "check_size": len(field),
                       "dict_byte": filters[-1][1][0] if filters and filters[-1][1] else 0})
        out += field
        real.append((len(header) + len(comp) + check_size, len(p)))
    recs = real if records is None else records
    index = bytes([indicator]) + _integer(len(recs) if count is None else count) + b"".join(_integer(a) + _integer(u) for a, u in recs)
    index += _pad4(len(index)) if index_padding is None else bytes(index_padding)
    index += struct.pack("<I", zlib.crc32(index) & 0xFFFFFFFF if index_crc is None else index_crc)
    out += index
    tail = struct.pack("<I", (len(index) // 4 - 1) & 0xFFFFFFFF if backward is None else backward) + (flags if footer_flags is None else bytes(footer_flags))
    out += struct.pack("<I", zlib.crc32(tail) & 0xFFFFFFFF if footer_crc is None else footer_crc) + tail + footer_magic + bytes(padding)
    return Built(bytes(out), layout)


def cut(payload, block):
    """`payload` in pieces of `block` bytes, the last one short (or none for an empty payload)."""
    return [payload[i:i + block] for i in range(0, len(payload), block)]
