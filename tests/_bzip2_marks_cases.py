"""bzip2 blocks and ends of streams found without a decode: an independent statement of the mark rule (include/swc_hip.h,
swc_index_blocks kind 10) and the buffers the three implementations -- the emulation of csrc/bzip2_scan.h, the host index, the
device call -- are held to it on.  TEST INFRASTRUCTURE ONLY."""
import random
import struct

BLOCK, END = 0x314159265359, 0x177245385090
END_FLAG = 1
_MAGICS = ((BLOCK.to_bytes(6, "big"), 0), (END.to_bytes(6, "big"), END_FLAG))


def bits_at(b, bit, count):
    """`count` bits of `b` from bit offset `bit`, MSB-first (all of them inside b)."""
    lo, hi = bit >> 3, (bit + count + 7) >> 3
    return (int.from_bytes(b[lo:hi], "big") >> (8 * hi - bit - count)) & ((1 << count) - 1)


def rule(b):
    """Every mark of `b` as (offset, comp_len, uncomp_len, aux, flags), in ascending order of the offset.  The buffer as one big
    integer shifted by s = 0..7 bits brings every bit offset 8 i + s onto byte i, where bytes.find sees it; then the two bounds."""
    b = bytes(b)
    L = 8 * len(b)
    whole = int.from_bytes(b, "big")
    found = []
    for s in range(8):
        shifted = ((whole << s) & ((1 << L) - 1)).to_bytes(len(b), "big")
        for magic, flag in _MAGICS:
            i = shifted.find(magic)
            while i >= 0:
                at = 8 * i + s
                if at >= 32 and at + 80 <= L:
                    found.append((at, flag))
                i = shifted.find(magic, i + 1)
    found.sort()
    ends = [at for at, _ in found[1:]] + [L]
    return [(at, nxt - at, 0, bits_at(b, at + 48, 32), flag) for (at, flag), nxt in zip(found, ends)]


def pack_refs(refs):
    return b"".join(struct.pack("<QQQII", *r) for r in refs)


# ---- buffers --------------------------------------------------------------------------------------------------------------------
def noise(n, seed):
    return bytearray(random.Random(0xB2 * 1000003 + seed).randbytes(n))


def put(buf, bit, value, count):
    """`count` bits of `value` into `buf` at bit offset `bit`, MSB-first."""
    lo, hi = bit >> 3, (bit + count + 7) >> 3
    shift = 8 * hi - bit - count
    old = int.from_bytes(buf[lo:hi], "big")
    new = (old & ~(((1 << count) - 1) << shift)) | (value << shift)
    buf[lo:hi] = new.to_bytes(hi - lo, "big")


def plant(buf, bit, magic=BLOCK, word=None):
    """A mark at `bit`: the magic and a word behind it (by default one that names the place)."""
    put(buf, bit, magic, 48)
    put(buf, bit + 48, (0xC0DE0000 ^ bit) & 0xFFFFFFFF if word is None else word, 32)


def _borders(border, count, tile, seed):
    """Marks that straddle `count` multiples of `border`: for every bit s = 0..7 one whose first byte lies 1, 3 and 6 bytes in front of
    a border -- and, the buffer being run at all 16 residues, at every other distance up to 21 as well."""
    n = border * (count + 1) + 40
    buf = noise(n, seed)
    k = 1
    for s in range(8):
        for d in (1, 3, 6):
            plant(buf, 8 * (border * k * (2 if border == 16 else 1) - d) + s, END if (s + d) % 4 == 0 else BLOCK)
            k += 1
    return bytes(buf)


def all_cases(tile):
    """[(name, buffer)]: the list the emulation, the host index and the device call share."""
    c = []
    c.append(("length 0", b""))
    b = noise(13, 1)
    plant(b, 24)
    c.append(("length 13", bytes(b)))
    b = noise(14, 2)
    plant(b, 32)
    c.append(("length 14, mark at bit 32", bytes(b)))
    b = noise(14, 3)
    plant(b, 31)
    c.append(("magic at bit 31", bytes(b)))
    b = noise(40, 4)
    plant(b, 31, END)
    plant(b, 8 * 40 - 80 - 3)
    c.append(("end magic at bit 31, a mark behind", bytes(b)))
    for n in (14, 15, 31, 33, 100, 1024 + 9, tile - 1, tile, tile + 1, tile + 10, 2 * tile + 7):   # the last mark a buffer can hold
        b = noise(n, 10 + n)
        plant(b, 8 * n - 80, END if n % 2 else BLOCK)
        c.append(("mark ends with the buffer, %d" % n, bytes(b)))
        if n >= 15:
            b = noise(n, 10 + n)
            put(b, 8 * n - 79, BLOCK, 48)
            c.append(("one bit too late, %d" % n, bytes(b)))
            for s in range(1, 8):   # b + 80 == L only at s = 0: at the other s the last mark ends s bits in front of the end
                b = noise(n, 20 + n + s)
                plant(b, 8 * n - 88 + s)
                if 8 * n - 88 + s >= 32:
                    c.append(("last mark at bit %d of its byte, %d" % (s, n), bytes(b)))
    b = noise(16 * 200 + 64, 5)
    for s in range(8):
        plant(b, 8 * (100 + 400 * s) + s, BLOCK)
        plant(b, 8 * (300 + 400 * s) + s, END)
    c.append(("every alignment, both magics", bytes(b)))
    c.append(("chunk borders", _borders(16, 48, tile, 6)))
    c.append(("step borders", _borders(1024, 24, tile, 7)))
    c.append(("tile borders", _borders(tile, 24, tile, 8)))
    b = noise(300, 9)
    plant(b, 35)
    plant(b, 35 + 80, BLOCK)
    plant(b, 8 * 100 + 6, BLOCK)
    plant(b, 8 * 110 + 6, END)
    c.append(("80 bits apart", bytes(b)))
    b = noise(5000, 11)
    plant(b, 32, BLOCK, 0x12345678)
    plant(b, 8 * 4321 + 5, END, 0x12345678)
    c.append(("a block, then the end", bytes(b)))
    b = noise(16 * 64 * 3, 12)   # the four bytes behind the first are a magic's at bit s, the 48 bits are not: bit 0 or bit 47 of it wrong
    for s in range(8):
        at = 8 * (64 + 160 * s) + s
        put(b, at, BLOCK ^ (1 << 47), 48)
        put(b, at + 8 * 50, END ^ 1, 48)
        put(b, at + 8 * 100, (BLOCK >> 8 << 8) | 0x58, 48)
    plant(b, 8 * 2000 + 3)
    c.append(("the first test alone is met", bytes(b)))
    n = 70 * tile + 123   # more than 64 tiles: the wave that sums the tile counts takes a second turn; tiles without marks between
    b = noise(n, 13)
    for t, s in ((0, 1), (0, 6), (2, 0), (63, 7), (64, 2), (64, 3), (65, 4), (69, 5)):
        plant(b, 8 * (t * tile + 100 * s + 50) + s, END if t == 65 else BLOCK)
    plant(b, 8 * n - 80 - 8 * 20)
    c.append(("more than 64 tiles", bytes(b)))
    c.append(("a megabyte of noise", bytes(noise(1 << 20, 14))))
    dense = bytearray(b"BZh9")
    for i in range(300):
        dense += (BLOCK if i % 7 else END).to_bytes(6, "big") + struct.pack(">I", i)
    c.append(("bare marks, 80 bits apart", bytes(dense)))
    return c


CAP_CASES = ("every alignment, both magics", "bare marks, 80 bits apart", "tile borders", "80 bits apart")


def caps(n):
    return (0, 1, n - 1, n, n + 5)


# ---- real streams: where the sequential walk of the model arrives ------------------------------------------------------------------
def walked_marks(data):
    """(offset, flags, aux) of every mark BZip2.multiDecompress arrives at in `data` -- streams back to back, all of them clean -- by the
    model of tests/_bzip2_build.py."""
    import _bzip2_build as B
    r, out = B._Bits(data), []
    while r.p < 8 * len(data):
        assert r.get(32) >> 8 == 0x425A68
        while True:
            at = r.p
            magic, word = r.get(48), r.get(32)
            out.append((at, END_FLAG if magic == END else 0, word))
            if magic == END:
                break
            assert magic == BLOCK and B.model_block(r)[0] == 0
        r.p = (r.p + 7) // 8 * 8
    return out
