"""Containers written field by field: gzip members (RFC 1952; what GzipHeader.swift:68-199 and GzipArchive.swift:79-100 read), zlib
streams (RFC 1950; ZlibHeader.swift:47-92, ZlibArchive.swift:25-42), LZ4 frames, legacy frames and skippable frames (LZ4.swift:73-330)
and bzip2 streams assembled over whole blocks (BZip2.swift:50-95).  Every field is an argument whose default is the valid value: one
call makes a valid archive, one changed argument a precise fault.  (.xz streams: _xz_build.stream.)  TEST INFRASTRUCTURE ONLY.  The
builders check nothing: what they write may be invalid on purpose, and what an archive means is for the cases to say."""
import struct
import zlib

from swcompression_amd import corpus


class Built(bytes):
    """The archive's bytes, with .layout: what the builder knows about where its parts lie."""
    layout = None

    @classmethod
    def of(cls, data, **layout):
        b = cls(data)
        b.layout = layout
        return b


# ------------------------------------------------------------------------------------------------------------------- Deflate bodies
def deflate_raw(payload, level=6):
    return corpus.deflate_raw(bytes(payload), level)


def deflate_flushed(payload, every=2048, full=True, level=6):
    """A raw stream with an empty stored block (Z_FULL_FLUSH; full=False: Z_SYNC_FLUSH, so that the pieces share history) behind
    every `every` bytes of the payload: what "deflate_unit_bytes" cuts into units."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    out = []
    for o in range(0, len(payload), every):
        out.append(c.compress(payload[o:o + every]))
        if o + every < len(payload):
            out.append(c.flush(zlib.Z_FULL_FLUSH if full else zlib.Z_SYNC_FLUSH))
    out.append(c.flush())
    return b"".join(out)


def deflate_stored(payload, final=True):
    """One stored block."""
    assert len(payload) < 65536
    return bytes([1 if final else 0]) + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + bytes(payload)


def deflate_mid_byte(payload):
    """A stream whose last block ends in the middle of a byte: one static-Huffman block of literals (RFC 1951 3.2.6), written here
    bit by bit.  Literals 0..143 take 8 bits, the end of the block 7, the block header 3: 8 n + 10 bits, never a whole byte."""
    assert all(b < 144 for b in payload)
    bits = [1, 1, 0]                                        # BFINAL = 1, BTYPE = 01 (least significant bit first)
    for b in payload:
        code = 0x30 + b
        bits += [(code >> (7 - i)) & 1 for i in range(8)]   # Huffman codes go out most significant bit first
    bits += [0] * 7                                         # end of block: 0000000
    assert len(bits) % 8 != 0
    out = bytearray((len(bits) + 7) // 8)
    for i, bit in enumerate(bits):
        out[i >> 3] |= bit << (i & 7)
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------------------------ gzip
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 0x01, 0x02, 0x04, 0x08, 0x10


def gzip_member(payload=b"", body=None, level=6, magic=b"\x1f\x8b", method=8, flags=None, ftext=False, reserved=0, mtime=0, xfl=0, os=255,
                extra=None, xlen=None, name=None, name_terminated=True, comment=None, comment_terminated=True, fhcrc=False,
                crc=None, isize=None, cut=None):
    """One member.  flags: None = what the parts below ask for, | FTEXT, | reserved (bits 5-7).  extra: [(si1, si2, bytes)] or
    [(si1, si2, bytes, length field)]; xlen: None = the length of what is written.  name / comment: bytes without the zero byte, which
    *_terminated adds.  fhcrc: True = the low 16 bits of the CRC-32 of the header as written, or the 16-bit value itself.  body: the
    raw Deflate stream, None = zlib's at `level`.  crc / isize: None = those of the payload.  cut: the member is cut to this many
    bytes (negative: from the end)."""
    payload = bytes(payload)
    if flags is None:
        flags = ((FEXTRA if extra is not None else 0) | (FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0) |
                 (FHCRC if fhcrc is not False else 0) | (FTEXT if ftext else 0) | reserved)
    h = bytearray(magic) + bytes([method, flags]) + struct.pack("<I", mtime) + bytes([xfl, os])
    if extra is not None:
        fields = bytearray()
        for f in extra:
            si1, si2, data = f[0], f[1], bytes(f[2])
            si1 = si1 if isinstance(si1, int) else ord(si1)
            si2 = si2 if isinstance(si2, int) else ord(si2)
            fields += bytes([si1, si2]) + struct.pack("<H", f[3] if len(f) > 3 else len(data)) + data
        h += struct.pack("<H", len(fields) if xlen is None else xlen) + fields
    if name is not None:
        h += bytes(name) + (b"\0" if name_terminated else b"")
    if comment is not None:
        h += bytes(comment) + (b"\0" if comment_terminated else b"")
    if fhcrc is not False:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xFFFF) if fhcrc is True else fhcrc)
    if body is None:
        body = deflate_raw(payload, level)
    trailer = struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF if crc is None else crc, len(payload) & 0xFFFFFFFF if isize is None else isize)
    whole = bytes(h) + bytes(body) + trailer
    if cut is not None:
        whole = whole[:cut]
    return Built.of(whole, header=len(h), body=len(body), isize=struct.unpack("<I", trailer[4:])[0], size=len(whole))


def bgzf_member(payload, bsize=None, bc_len=None, before=(), behind=(), **kw):
    """A member with the 'BC' field of BGZF beside the sub-fields `before` and `behind`; bsize: None = the member's size - 1."""
    def make(value):
        bc = ("B", "C", struct.pack("<H", value)) if bc_len is None else ("B", "C", struct.pack("<H", value) + bytes(max(bc_len - 2, 0)), bc_len)
        if bc_len is not None and bc_len < 2:
            bc = ("B", "C", struct.pack("<H", value)[:bc_len], bc_len)
        return gzip_member(payload, extra=list(before) + [bc] + list(behind), **kw)
    size = len(make(0))
    assert size <= 65536
    return make(size - 1 if bsize is None else bsize)


# ------------------------------------------------------------------------------------------------------------------------------ zlib
def adler32(data):
    return zlib.adler32(bytes(data)) & 0xFFFFFFFF


def zlib_stream(payload=b"", body=None, level=6, cm=8, cinfo=7, flevel=2, fdict=False, dictid=b"\0\0\0\0", fcheck=None, adler=None,
                trailer=None):
    """cm, cinfo: the nibbles of CMF; flevel: bits 6-7 of FLG; fdict: bit 5, with `dictid` (any number of bytes) behind the header;
    fcheck: None = what makes CMF * 256 + FLG a multiple of 31; adler: None = the payload's; trailer: the bytes behind the body
    instead of the four of the Adler-32."""
    payload = bytes(payload)
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (0x20 if fdict else 0)
    if fcheck is None:
        fcheck = (31 - ((cmf << 8) + flg) % 31) % 31
    flg |= fcheck
    head = bytes([cmf & 0xFF, flg & 0xFF]) + (bytes(dictid) if fdict else b"")
    if body is None:
        body = deflate_raw(payload, level)
    if trailer is None:
        trailer = struct.pack(">I", adler32(payload) if adler is None else adler)
    return Built.of(head + bytes(body) + bytes(trailer), header=len(head), body=len(body))


# ------------------------------------------------------------------------------------------------------------------------------- LZ4
LZ4_MAGIC, LZ4_LEGACY_MAGIC, LZ4_SKIPPABLE_MAGIC = 0x184D2204, 0x184C2102, 0x184D2A50
xxh32 = corpus._xxh32


def lz4_literals(payload):
    """A compressed block that is one sequence of literals (what the block format asks of a block's last sequence)."""
    import _lz4_build
    return _lz4_build.block([], bytes(payload))


def lz4_frame(blocks=(), version=1, independent=True, block_checksum=False, content_size=None, content_checksum=None, reserved=0,
              dict_id=None, bd=0x70, flg=None, header_checksum=None, end_mark=True, magic=LZ4_MAGIC, cut=None):
    """blocks: [(bytes, stored)] or [(bytes, stored, size word, checksum)] -- a size word or checksum of None is the right one, the
    checksum is written only where block_checksum is set.  content_size / dict_id: None = no such field (an int: the field and its
    FLG bit).  content_checksum: None = no such field, an int = the four bytes behind the end mark, bytes = written as they are (a cut
    field).  flg: the whole byte instead of the bits.  header_checksum: None = the right byte."""
    if flg is None:
        flg = ((version & 3) << 6 | (0x20 if independent else 0) | (0x10 if block_checksum else 0) | (0x08 if content_size is not None else 0) |
               (0x04 if content_checksum is not None else 0) | (0x02 if reserved else 0) | (0x01 if dict_id is not None else 0))
    desc = bytes([flg, bd])
    if content_size is not None:
        desc += struct.pack("<Q", content_size)
    if dict_id is not None:
        desc += struct.pack("<I", dict_id)
    out = bytearray(struct.pack("<I", magic) + desc)
    out.append((xxh32(desc) >> 8) & 0xFF if header_checksum is None else header_checksum)
    refs = []
    for b in blocks:
        data, stored = bytes(b[0]), b[1]
        word = b[2] if len(b) > 2 and b[2] is not None else (len(data) | (0x80000000 if stored else 0))
        out += struct.pack("<I", word)
        refs.append((len(out), len(data), 0, 1 if stored else 0))
        out += data
        if block_checksum:
            out += struct.pack("<I", b[3] if len(b) > 3 and b[3] is not None else xxh32(data))
    if end_mark:
        out += struct.pack("<I", 0)
    if content_checksum is not None:
        out += content_checksum if isinstance(content_checksum, bytes) else struct.pack("<I", content_checksum)
    whole = bytes(out) if cut is None else bytes(out)[:cut]
    return Built.of(whole, blocks=refs, linked=not (flg & 0x20))


def lz4_legacy(blocks=(), magic=LZ4_LEGACY_MAGIC):
    """blocks: [bytes] or [(bytes, size word)]."""
    out = bytearray(struct.pack("<I", magic))
    for b in blocks:
        data, word = (bytes(b), None) if isinstance(b, (bytes, bytearray)) else (bytes(b[0]), b[1])
        out += struct.pack("<I", len(data) if word is None else word) + data
    return Built.of(bytes(out))


def lz4_skippable(data=b"", nibble=0, size=None):
    return Built.of(struct.pack("<II", LZ4_SKIPPABLE_MAGIC + nibble, len(data) if size is None else size) + bytes(data))


# ----------------------------------------------------------------------------------------------------------------------------- bzip2
BZ_BLOCK, BZ_END = 0x314159265359, 0x177245385090


class Bits:
    """Most significant bit first, as bzip2 writes."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, count):
        self.v = (self.v << count) | (value & ((1 << count) - 1))
        self.n += count
        return self

    def bits(self):
        return self.v, self.n

    def bytes(self):
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def bzip2_blocks(stream):
    """The blocks of a stream libbz2 wrote, each as (crc, body bits as (value, count)): found by their marks (a test stream is small
    enough for a mark inside a block's data not to occur; the stream CRC read back is checked against the blocks')."""
    total = len(stream) * 8
    v = int.from_bytes(stream, "big")
    def at(bit, count):
        return (v >> (total - bit - count)) & ((1 << count) - 1)
    marks = [b for b in range(32, total - 47) if at(b, 48) in (BZ_BLOCK, BZ_END)]
    blocks, combined = [], 0
    for k, m in enumerate(marks):
        if at(m, 48) == BZ_END:
            assert at(m + 48, 32) == combined
            break
        crc = at(m + 48, 32)
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ crc
        blocks.append((crc, (at(m + 80, marks[k + 1] - m - 80), marks[k + 1] - m - 80)))
    return blocks


def bzip2_stream(blocks, head=b"BZh9", crcs=None, marks=None, stream_crc=None, end_mark=BZ_END, behind=b"", tail_bits=None):
    """blocks: what bzip2_blocks gives.  crcs: the stored block CRCs, None = the blocks' own; marks: the 48 bits in front of each
    block; stream_crc: None = combined from the STORED block CRCs, as the reader combines them (BZip2.swift:83-84); end_mark: the 48
    bits of the end of the stream, None = no end at all; tail_bits: the whole stream is cut to this many bits behind the last block
    (the bits of the end mark and CRC as far as they go); behind: bytes behind the padded stream."""
    w = Bits()
    for c in head:
        w.put(c, 8)
    combined, starts = 0, []
    for k, (crc, (body, n)) in enumerate(blocks):
        stored = crc if crcs is None or crcs[k] is None else crcs[k]
        starts.append(w.n)
        w.put(BZ_BLOCK if marks is None or marks[k] is None else marks[k], 48).put(stored, 32).put(body, n)
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ stored
    end_at = w.n
    if end_mark is not None:
        t = Bits().put(end_mark, 48).put(combined if stream_crc is None else stream_crc, 32)
        tv, tn = t.bits()
        if tail_bits is not None:
            tv, tn = tv >> (tn - tail_bits), tail_bits
        w.put(tv, tn)
    return Built.of(w.bytes() + bytes(behind), blocks=starts, end=end_at)
