"""An LZMA2 stream taken apart into chunks and PACKETS (TEST INFRASTRUCTURE; standard library only).

A decoder written from the format for the tests of the encoder (csrc/lzma_comp.h): it does not return the bytes alone, as liblzma
and the oracle do, but what the encoder DECIDED -- every chunk's control byte and sizes, and every packet with its kind, length,
distance and the rep0 that was in force in front of it.  Fed to tests/_lzma_build.py's Builder, an independent range encoder, the
same list must give the same bytes.  It reads what an LZMA2 writer of one dictionary may write (properties lc + lp <= 4, all
packet kinds, all six controls); it is no validator: a damaged stream ends in an exception.
"""
import collections

# kind: "literal" | "match" | "rep0" .. "rep3" | "shortrep"; distance: bytes back (0 for a literal); rep0: the decoder's rep0 in front
# of the packet; pos: the output position of its first byte; byte: a literal's value
Packet = collections.namedtuple("Packet", "kind length distance rep0 pos byte")
# control: the byte; start / unpack: the chunk's bytes in the output; comp: payload bytes (None: stored); props: (lc, lp, pb) where written
Chunk = collections.namedtuple("Chunk", "control start unpack comp props packets")


class _Range:
    def __init__(self, data):
        assert len(data) >= 5 and data[0] == 0
        self.d, self.at = data, 5
        self.range, self.code = 0xFFFFFFFF, int.from_bytes(data[1:5], "big")

    def _norm(self):
        if self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.code = ((self.code << 8) | self.d[self.at]) & 0xFFFFFFFF
            self.at += 1

    def bit(self, cells, i):
        p = cells[i]
        bound = (self.range >> 11) * p
        if self.code < bound:
            self.range = bound
            cells[i] = p + ((2048 - p) >> 5)
            b = 0
        else:
            self.range -= bound
            self.code -= bound
            cells[i] = p - (p >> 5)
            b = 1
        self._norm()
        return b

    def direct(self, n):
        v = 0
        for _ in range(n):
            self.range >>= 1
            b = 1 if self.code >= self.range else 0
            if b:
                self.code -= self.range
            self._norm()
            v = (v << 1) | b
        return v

    def tree(self, cells, base, n):
        m = 1
        for _ in range(n):
            m = (m << 1) | self.bit(cells, base + m)
        return m - (1 << n)

    def rtree(self, cells, base, n):
        m, v = 1, 0
        for i in range(n):
            b = self.bit(cells, base + m)
            m = (m << 1) | b
            v |= b << i
        return v


class _Model:
    def __init__(self, lc, lp, pb):
        self.lc, self.lp, self.pb = lc, lp, pb
        self.reset()

    def reset(self):
        I = 1024
        self.is_match, self.rep0_long = [I] * 192, [I] * 192
        self.is_rep, self.g0, self.g1, self.g2 = [I] * 12, [I] * 12, [I] * 12, [I] * 12
        self.slot = [[I] * 64 for _ in range(4)]
        self.special, self.align = [I] * 115, [I] * 16
        self.len, self.rep_len = ([I] * 258, [I] * 256), ([I] * 258, [I] * 256)
        self.lit = {}
        self.state, self.reps = 0, [0, 0, 0, 0]


def _length(rc, coder, ps):
    low, high = coder
    if rc.bit(low, 0) == 0:
        return rc.tree(low, 2 + ps * 8, 3)
    if rc.bit(low, 1) == 0:
        return 8 + rc.tree(low, 2 + 128 + ps * 8, 3)
    return 16 + rc.tree(high, 0, 8)


def _chunk_packets(rc, m, out, unpack, dict_start, packets):
    end = len(out) + unpack
    while len(out) < end:
        pos = len(out)
        ps = pos & ((1 << m.pb) - 1)
        s, rep0 = m.state, m.reps[0]
        if rc.bit(m.is_match, (s << 4) + ps) == 0:
            prev = 0 if pos == dict_start else out[-1]
            ls = ((pos & ((1 << m.lp) - 1)) << m.lc) + (prev >> (8 - m.lc))
            cells = m.lit.setdefault(ls, [1024] * 0x300)
            sym = 1
            if s >= 7:
                mb = out[pos - rep0 - 1]
                while sym < 0x100:
                    mbit = (mb >> 7) & 1
                    mb = (mb << 1) & 0xFF
                    b = rc.bit(cells, ((1 + mbit) << 8) + sym)
                    sym = (sym << 1) | b
                    if mbit != b:
                        break
            while sym < 0x100:
                sym = (sym << 1) | rc.bit(cells, sym)
            out.append(sym & 0xFF)
            packets.append(Packet("literal", 1, 0, rep0, pos, sym & 0xFF))
            m.state = 0 if s < 4 else s - 3 if s < 10 else s - 6
            continue
        if rc.bit(m.is_rep, s) == 0:
            n = _length(rc, m.len, ps)
            slot = rc.tree(m.slot[min(n, 3)], 0, 6)
            if slot < 4:
                r = slot
            else:
                ndb = (slot >> 1) - 1
                base = (2 | (slot & 1)) << ndb
                if slot < 14:
                    r = base + rc.rtree(m.special, base - slot, ndb)
                else:
                    r = base + (rc.direct(ndb - 4) << 4)
                    r += rc.rtree(m.align, 0, 4)
            m.reps = [r] + m.reps[:3]
            m.state = 7 if s < 7 else 10
            kind, length = "match", n + 2
        else:
            if rc.bit(m.g0, s) == 0:
                if rc.bit(m.rep0_long, (s << 4) + ps) == 0:
                    out.append(out[pos - rep0 - 1])
                    packets.append(Packet("shortrep", 1, rep0 + 1, rep0, pos, None))
                    m.state = 9 if s < 7 else 11
                    continue
                i = 0
            elif rc.bit(m.g1, s) == 0:
                i = 1
            else:
                i = 2 + rc.bit(m.g2, s)
            m.reps.insert(0, m.reps.pop(i))
            kind, length = "rep%d" % i, _length(rc, m.rep_len, ps) + 2
            m.state = 8 if s < 7 else 11
        d = m.reps[0] + 1
        assert d <= pos - dict_start, "a match reaches in front of the dictionary"
        assert pos + length <= end, "a packet crosses the chunk's end"
        for _ in range(length):
            out.append(out[-d])
        packets.append(Packet(kind, length, d, rep0, pos, None))


def parse(stream):
    """stream: raw LZMA2 (no dictionary-size byte).  Returns (chunks, plain bytes, bytes consumed, end marker met)."""
    out, chunks, at = bytearray(), [], 0
    m, dict_start = None, 0
    while at < len(stream):
        c = stream[at]
        if c == 0:
            return chunks, bytes(out), at + 1, True
        if c in (1, 2):
            n = (stream[at + 1] << 8) + stream[at + 2] + 1
            if c == 1:
                dict_start = len(out)
            chunks.append(Chunk(c, len(out), n, None, None, []))
            out += stream[at + 3:at + 3 + n]
            assert len(out) == chunks[-1].start + n
            at += 3 + n
            continue
        assert c >= 0x80, "control byte %#x" % c
        unpack = ((c & 0x1F) << 16) + (stream[at + 1] << 8) + stream[at + 2] + 1
        comp = (stream[at + 3] << 8) + stream[at + 4] + 1
        at += 5
        props = None
        reset = (c >> 5) & 3
        if reset >= 2:
            b = stream[at]
            at += 1
            props = (b % 9, (b // 9) % 5, b // 45)
            m = _Model(*props)
        elif reset == 1:
            m.reset()
        if reset == 3:
            dict_start = len(out)
        packets = []
        rc = _Range(stream[at:at + comp])
        start = len(out)
        _chunk_packets(rc, m, out, unpack, dict_start, packets)
        assert rc.at == comp and rc.code == 0, "the payload is not the range coder's with its flush"
        chunks.append(Chunk(c & 0xE0, start, unpack, comp, props, packets))
        at += comp
    return chunks, bytes(out), at, False
