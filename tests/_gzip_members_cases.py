"""Plain gzip members found without a decode: an independent statement of the candidate rule (include/swc_hip.h, swc_index_blocks kind
9) and the buffers the three implementations -- the emulation of csrc/gzip_scan.h, the host index, the device call -- are held to it
on.  TEST INFRASTRUCTURE ONLY."""
import random
import re
import struct

UNUSABLE = 1
_START = re.compile(rb"(?=\x1f\x8b\x08[\x00-\x1f])", re.S)


def data_pos(b, p):
    """Where the data of the member at p would start, or None: the header leaves the buffer or a name is over 256 bytes."""
    flags, q = b[p + 3], p + 10
    if flags & 4:
        if q + 2 > len(b):
            return None
        q += 2 + b[q] + 256 * b[q + 1]
    for bit in (8, 16):
        if flags & bit:
            z = b.find(b"\0", q, q + 256)
            if z < 0:
                return None
            q = z + 1
    if flags & 2:
        q += 2
    return q if q <= len(b) else None


def rule(b):
    """Every candidate of `b` as (offset, comp_len, uncomp_len, aux, flags), in file order."""
    b = bytes(b)
    starts = [m.start() for m in _START.finditer(b) if m.start() + 20 <= len(b)]
    refs = []
    for p, nxt in zip(starts, starts[1:] + [len(b)]):
        q = data_pos(b, p)
        if q is None or q + 10 > nxt:
            refs.append((p, 0, 0, 0, UNUSABLE))
        else:
            refs.append((q, nxt - q - 8, struct.unpack_from("<I", b, nxt - 4)[0], q - p, 0))
    return refs


def pack_refs(refs):
    return b"".join(struct.pack("<QQQII", *r) for r in refs)


# ---- buffers --------------------------------------------------------------------------------------------------------------------
EMPTY = bytes.fromhex("0300")   # an empty static block


def member(flags=0, body=EMPTY, extra=b"", name=b"", comment=b"", trailer=b"\x11\x22\x33\x44\x55\x66\x77\x88", xlen=None):
    """The bytes of a member as the rule sees it: header fields by `flags` (FEXTRA with `extra`, the names with their zero), the body,
    eight trailer bytes.  xlen: the XLEN field, where it is not to be the length of `extra`."""
    h = bytes([0x1f, 0x8b, 8, flags, 0, 0, 0, 0, 0, 255])
    if flags & 4:
        h += struct.pack("<H", len(extra) if xlen is None else xlen) + extra
    if flags & 8:
        h += name + b"\0"
    if flags & 16:
        h += comment + b"\0"
    if flags & 2:
        h += b"\xab\xcd"
    return h + body + trailer


def filler(n, seed):
    """n bytes that hold no 0x1f: no candidate starts in them."""
    r = random.Random(seed)
    return bytes(r.choice(b"\x00\x01\x8b\x08\x20\xfe\xff") for _ in range(n))


def lengths(tile):
    """0..44, and every length within 20 bytes of one and of two tiles."""
    return list(range(45)) + [k * tile + d for k in (1, 2) for d in range(-20, 21)]


def of_length(n, late=False):
    """A buffer of exactly n bytes with members wherever they fit, short and long, the last one at exactly n - 20 -- or, `late`, at
    n - 19: too close to the end to be a candidate."""
    r = random.Random(n * 7)
    out = bytearray()
    while len(out) < n:
        out += member(r.choice((0, 1, 2, 8, 0x1f)), body=EMPTY + filler(r.randrange(0, 1500), len(out)), extra=b"ab\x02\x00xy", name=b"n", comment=b"c")
    out = out[:n]
    if late and n >= 19:
        out[n - 19:] = member()[:19]
    elif n >= 20:
        out[n - 20:] = member()
    return bytes(out)


def dense(n):
    return (b"\x1f\x8b\x08" * (n // 3 + 1))[:n]


def soak(n, seed):
    r = random.Random(seed)
    return bytes(r.choice(b"\x1f\x8b\x08\x00\x02\x04\x1c\xe0\xff") for _ in range(n))


def header_cases():
    """name -> buffer: what a header can be."""
    c = {}
    for f in range(32):   # every flag combination, a member behind each
        c["flags %02x" % f] = member(f, extra=b"AB\x03\x00xyz", name=b"file.txt", comment=b"hello") + member(0) + filler(7, f)
    c["xlen past the end"] = member(0) + member(4, extra=b"1234", xlen=60000)
    c["xlen to the last byte"] = member(4, extra=b"x" * 9, body=b"", trailer=b"")[:20] + b"y"
    for k in (255, 256, 257):   # bytes of the name with its zero
        c["name of %d" % k] = member(8, name=b"n" * (k - 1)) + member(0)
        c["comment of %d" % k] = member(0x18, name=b"x", comment=b"c" * (k - 1)) + member(0)
    c["name holds the magic"] = member(8, name=b"a\x1f\x8b\x08\x08b") + member(0)
    c["name without a zero"] = filler(3, 3) + b"\x1f\x8b\x08\x08" * 200
    c["header ends behind the next"] = member(4, extra=b"\x1f\x8b\x08\x00" + b"e" * 30) + member(0)
    c["next too close"] = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255, 3, 0]) + member(0) + member(0)
    c["last at len - 20"] = filler(33, 4) + member(0)
    c["none at len - 19"] = filler(33, 5) + member(0)[:19]
    c["last at len - 20, header longer"] = filler(9, 6) + member(0x1e, extra=b"", name=b"", comment=b"")[:20]
    c["isize words"] = member(0, trailer=struct.pack("<II", 0xDEADBEEF, 0x01020304)) + member(2, trailer=struct.pack("<II", 1, 0xFFFFFFFF))
    return c


def all_cases(tile):
    """[(name, buffer)]: the list the emulation, the host index and the device call share."""
    cases = [("length %d" % n, of_length(n)) for n in lengths(tile)]
    cases += [("length %d, late" % n, of_length(n, late=True)) for n in lengths(tile) if n >= 19]
    cases += sorted(header_cases().items())
    cases += [("dense %d" % n, dense(n)) for n in (19, 20, 21, 22, 23, 64, 1027, 3 * tile + 37)]
    cases += [("soak %d" % s, soak(3 * tile + 37, s)) for s in range(3)]
    return cases
