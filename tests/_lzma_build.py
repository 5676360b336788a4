"""LZMA / LZMA2 streams BUILT decision by decision (TEST INFRASTRUCTURE; standard library only).

liblzma is a narrow encoder: it never changes lc / lp / pb inside a stream, never resets the dictionary behind the first chunk,
never continues the model (0x80) behind a stored chunk, never writes lc + lp > 4, an end marker inside an LZMA2 chunk, a match
that reaches behind a dictionary reset or a dictionary of fewer than 4,096 bytes.  The reference accepts all of that, and so
must the kernels (swcompression_amd/csrc/lzma_wave.h).  This module writes such streams from the format: a range ENCODER (low /
range / cache with carry, adaptive 11-bit cells, direct bits, a five-byte flush), the encoder's copy of the decoder's model,
one method per packet kind, the LZMA2 chunk framing with every control byte, `random_stream` for the soak tests and
`directed_cases` for the named corners.  The builder keeps counters of what it wrote (packet kind x state, pos slot, length
tier x coder, chunk control, model shape), by which the self-check (test_lzma_build.py) proves coverage.

What the builder mirrors of the reference and liblzma does not do (or does differently):
  * pos_state and the literal coder are chosen from the TOTAL output position, the context byte of a literal is 0 whenever the
    output position equals the start of the dictionary (at offset 0, behind a 0xE0 chunk, always with a dictionary of one byte);
  * a match is legal when rep0 < dict_size and rep0 < output position -- whatever dictionary resets lie in between;
  * a long or short rep0 from state 11 at pos_state 15 (pb = 4) is a trap of the reference: `rep0_traps()`
    tells, valid streams steer around it;
  * 0xA0 as the FIRST chunk is legal: the model is built from the default properties lc 3, lp 0, pb 2.
`liblzma_ok` is decided by rule from the structure (never by asking liblzma): see `Builder._l2_rule` and `Builder.case`.
"""
import collections
import functools
import random

INIT = 1024
KINDS = ("literal", "match", "rep0", "rep1", "rep2", "rep3", "shortrep")
CONTROLS = (0x80, 0xA0, 0xC0, 0xE0)
TRAP, CAPACITY = 900, 901
WRONG_PROPERTIES, INIT_ERROR, EXCEEDED, WINDOW_EMPTY, FINISH_ERROR, WILL_EXCEED, NOT_ENOUGH = 301, 302, 303, 304, 305, 306, 307
WRONG_DICT, WRONG_CONTROL, WRONG_SIZES = 401, 402, 404

# kind: "lzma2" (dict_byte set, props None) or "lzma" (props = (lc, lp, pb, dict_size, declared_size), declared_size -1: unknown);
# plain: None for an error case; consumed: the input the decoder has read when it stops (valid cases); liblzma_ok: see above
Case = collections.namedtuple("Case", "name stream kind dict_byte props plain status consumed liblzma_ok")


class RangeEncoder:
    def __init__(self):
        self.low, self.range, self.cache, self.cache_size = 0, 0xFFFFFFFF, 0, 1
        self.out = bytearray()

    def _shift_low(self):
        if self.low < 0xFF000000 or self.low >> 32:
            carry = self.low >> 32
            self.out.append((self.cache + carry) & 0xFF)
            if self.cache_size > 1:
                self.out += bytes([(0xFF + carry) & 0xFF]) * (self.cache_size - 1)
            self.cache_size = 0
            self.cache = (self.low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def bit(self, cells, i, b):
        p = cells[i]
        bound = (self.range >> 11) * p
        if b:
            self.low += bound
            self.range -= bound
            cells[i] = p - (p >> 5)
        else:
            self.range = bound
            cells[i] = p + ((2048 - p) >> 5)
        if self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self._shift_low()

    def direct(self, value, nbits):
        for i in range(nbits - 1, -1, -1):
            self.range >>= 1
            if (value >> i) & 1:
                self.low += self.range
            if self.range < 1 << 24:
                self.range = (self.range << 8) & 0xFFFFFFFF
                self._shift_low()

    def tree(self, cells, base, nbits, value):
        m = 1
        for i in range(nbits - 1, -1, -1):
            b = (value >> i) & 1
            self.bit(cells, base + m, b)
            m = (m << 1) | b

    def tree_reverse(self, cells, base, nbits, value):
        m = 1
        for i in range(nbits):
            b = (value >> i) & 1
            self.bit(cells, base + m, b)
            m = (m << 1) | b

    def pending(self):
        return len(self.out) + self.cache_size

    def flush(self, offset=0):
        """Five bytes: the decoder's `code` ends as `offset` (0: the stream is finished; must stay below the range)."""
        assert offset < self.range
        self.low += offset
        for _ in range(5):
            self._shift_low()
        return bytes(self.out)


class Model:
    """The decoder's cells, as the encoder keeps them.  Literal coders are made when first used (lc + lp = 12 has 4,096)."""

    def __init__(self, lc, lp, pb):
        assert 0 <= lc <= 8 and 0 <= lp <= 4 and 0 <= pb <= 4
        self.lc, self.lp, self.pb = lc, lp, pb
        self.reset()

    def reset(self):
        self.is_match = [INIT] * (12 << 4)
        self.is_rep, self.g0, self.g1, self.g2 = [INIT] * 12, [INIT] * 12, [INIT] * 12, [INIT] * 12
        self.rep0_long = [INIT] * (12 << 4)
        self.pos_slot = [[INIT] * 64 for _ in range(4)]
        self.special = [INIT] * 115
        self.align = [INIT] * 16
        self.len = ([INIT] * 258, [INIT] * 256)       # choice, choice2, low[16][8], mid[16][8]; high[256]
        self.rep_len = ([INIT] * 258, [INIT] * 256)
        self.lit = {}
        self.state = 0
        self.reps = [0, 0, 0, 0]

    def props_byte(self):
        return (self.pb * 5 + self.lp) * 9 + self.lc


def pos_slot_of(rep0):
    if rep0 < 4:
        return rep0
    n = rep0.bit_length()
    return 2 * (n - 1) + ((rep0 >> (n - 2)) & 1)


def slot_base(slot):
    return slot if slot < 4 else (2 | (slot & 1)) << ((slot >> 1) - 1)


def lzma2_dict_size(dict_byte):
    return max(4096, (2 | (dict_byte & 1)) << (dict_byte // 2 + 11))


class Builder:
    """One stream.  kind "lzma2": chunk() / stored() frame the packets, case() closes the last chunk and writes the terminator.  kind "lzma": the
    packets are the stream.  Every packet method appends to the plain text; once a packet has been written that the reference
    answers with an error (`status` says which), nothing more may follow."""

    def __init__(self, kind, dict_byte=None, props=None, dict_size=None, declared=-1, counters=None, auto_split=True):
        assert kind in ("lzma2", "lzma")
        self.kind, self.dict_byte, self.declared = kind, dict_byte, declared
        self.out = bytearray()
        self.dict_start = 0
        self.reset_at = 0            # where the dictionary was last reset (dict_start also moves when the window slides)
        self.status = 0
        self.count = collections.Counter() if counters is None else counters
        self.ok = True               # liblzma decodes this (by rule)
        self.refused = set()         # the liblzma-refused constructs met
        self.end_marked = False
        self.auto_split = auto_split
        if kind == "lzma2":
            self.dict_size = lzma2_dict_size(dict_byte)
            self.stream = bytearray()
            self.m, self.rc, self.control = None, None, None
            self.need_dict_reset, self.need_props = True, True
        else:
            self.dict_size = dict_size
            self.m = Model(*props)
            self.rc = RangeEncoder()
            self.count["shape", props[0], props[1], props[2]] += 1
            if props[0] + props[1] > 4:
                self._refuse("lc+lp>4")
            if dict_size < 4096:
                self._refuse("small dictionary")

    # ---- bookkeeping ------------------------------------------------------------------------------------------------
    def _refuse(self, why):
        self.ok = False
        self.refused.add(why)

    def _fail(self, status):
        assert self.status == 0
        self.status = status

    def _put(self, data):
        self.out += data
        if self.dict_size > 0 and len(self.out) - self.dict_start >= self.dict_size:
            self.dict_start = len(self.out) - self.dict_size + 1

    def _packet(self, kind):
        assert self.status == 0 and self.rc is not None and not self.end_marked, "nothing follows an error or an end marker"
        if self.kind == "lzma2" and self.auto_split and (self.rc.pending() > 60000 or len(self.out) - self.chunk_start > (1 << 21) - 300):
            self.chunk(0x80)
        self.count["packet", kind, self.m.state] += 1
        pos = len(self.out)
        return self.m, self.rc, pos, pos & ((1 << self.m.pb) - 1)

    def pos_state(self):
        return len(self.out) & ((1 << self.m.pb) - 1)

    def rep0_traps(self):
        """A long or short rep0 here indexes the cell the reference does not have (state 11, pos_state 15)."""
        return (self.m.state << 4) + self.pos_state() >= 191

    def window_empty(self):
        return len(self.out) == self.dict_start

    def match_ok(self, distance):
        return 1 <= distance <= len(self.out) and distance - 1 < self.dict_size

    def _since_reset(self, distance):
        if distance > len(self.out) - self.reset_at:
            self._refuse("distance behind a dictionary reset")

    # ---- packets ----------------------------------------------------------------------------------------------------
    def literal(self, b):
        m, rc, pos, ps = self._packet("literal")
        rc.bit(m.is_match, (m.state << 4) + ps, 0)
        prev = 0 if pos == self.dict_start else self.out[-1]
        ls = ((pos & ((1 << m.lp) - 1)) << m.lc) + (prev >> (8 - m.lc))
        cells = m.lit.get(ls)
        if cells is None:
            cells = m.lit[ls] = [INIT] * 0x300
        self.count["coder", ls] += 1
        symbol = 1
        matched = m.state >= 7
        mb = self.out[pos - m.reps[0] - 1] if matched else 0
        for i in range(7, -1, -1):
            bit = (b >> i) & 1
            if matched:
                mbit = (mb >> i) & 1
                rc.bit(cells, ((1 + mbit) << 8) + symbol, bit)
                matched = mbit == bit
            else:
                rc.bit(cells, symbol, bit)
            symbol = (symbol << 1) | bit
        self._put(bytes([b]))
        s = m.state
        m.state = 0 if s < 4 else s - 3 if s < 10 else s - 6

    def _len(self, coder, which, n, ps):
        low, high = coder
        rc = self.rc
        if n < 8:
            rc.bit(low, 0, 0)
            rc.tree(low, 2 + ps * 8, 3, n)
        elif n < 16:
            rc.bit(low, 0, 1)
            rc.bit(low, 1, 0)
            rc.tree(low, 2 + 128 + ps * 8, 3, n - 8)
        else:
            rc.bit(low, 0, 1)
            rc.bit(low, 1, 1)
            rc.tree(high, 0, 8, n - 16)
        self.count["len", which, "low" if n < 8 else "mid" if n < 16 else "high"] += 1
        self.count["len-value", which, n + 2] += 1
        if n < 16:
            self.count["len-pos-state", which, ps] += 1

    def _copy(self, distance, length):
        src = len(self.out) - distance
        if distance >= length:
            self._put(self.out[src:src + length])
        else:
            piece = bytes(self.out[src:])
            self._put((piece * (length // distance + 1))[:length])

    def match(self, distance, length):
        """A match with a distance of its own.  One that the reference refuses (distance beyond the dictionary or the output) is
        written all the same and ends the stream with the reference's status."""
        assert 2 <= length <= 273 and 1 <= distance <= 1 << 32
        m, rc, pos, ps = self._packet("match")
        rep0 = distance - 1
        rc.bit(m.is_match, (m.state << 4) + ps, 1)
        rc.bit(m.is_rep, m.state, 0)
        self._len(m.len, "len", length - 2, ps)
        slot = pos_slot_of(rep0)
        self.count["slot", slot] += 1
        rc.tree(m.pos_slot[min(length - 2, 3)], 0, 6, slot)
        if slot >= 4:
            ndb = (slot >> 1) - 1
            base = (2 | (slot & 1)) << ndb
            rem = rep0 - base
            if slot < 14:
                rc.tree_reverse(m.special, base - slot, ndb, rem)
            else:
                rc.direct(rem >> 4, ndb - 4)
                rc.tree_reverse(m.align, 0, 4, rem & 15)
        m.reps = [rep0] + m.reps[:3]
        m.state = 7 if m.state < 7 else 10
        if rep0 == 0xFFFFFFFF:
            self.end_marked = True
            if self.kind == "lzma2":
                self._refuse("end marker in a chunk")
            elif self.declared >= 0:
                self._refuse("end marker behind a declared size")   # (liblzma: depends on its version)
            return
        if rep0 >= self.dict_size or (rep0 > pos and pos < self.dict_size):
            return self._fail(NOT_ENOUGH)
        if rep0 + 1 > pos:
            return self._fail(TRAP)
        self._since_reset(distance)
        self._copy(distance, length)

    def end_marker(self, length=2):
        self.match(1 << 32, length)

    def rep(self, i, length):
        assert 0 <= i <= 3 and 2 <= length <= 273
        m, rc, pos, ps = self._packet("rep%d" % i)
        rc.bit(m.is_match, (m.state << 4) + ps, 1)
        rc.bit(m.is_rep, m.state, 1)
        if pos == self.dict_start:
            return self._fail(WINDOW_EMPTY)
        if i == 0:
            rc.bit(m.g0, m.state, 0)
            if (m.state << 4) + ps >= 191:
                return self._fail(TRAP)
            rc.bit(m.rep0_long, (m.state << 4) + ps, 1)
        else:
            rc.bit(m.g0, m.state, 1)
            rc.bit(m.g1, m.state, 0 if i == 1 else 1)
            if i > 1:
                rc.bit(m.g2, m.state, 0 if i == 2 else 1)
            d = m.reps.pop(i)
            m.reps.insert(0, d)
        self._len(m.rep_len, "rep_len", length - 2, ps)
        m.state = 8 if m.state < 7 else 11
        assert m.reps[0] + 1 <= pos, "a rep distance never exceeds the output"
        self._since_reset(m.reps[0] + 1)
        self._copy(m.reps[0] + 1, length)

    def short_rep(self):
        m, rc, pos, ps = self._packet("shortrep")
        rc.bit(m.is_match, (m.state << 4) + ps, 1)
        rc.bit(m.is_rep, m.state, 1)
        if pos == self.dict_start:
            return self._fail(WINDOW_EMPTY)
        rc.bit(m.g0, m.state, 0)
        if (m.state << 4) + ps >= 191:
            return self._fail(TRAP)
        rc.bit(m.rep0_long, (m.state << 4) + ps, 0)
        m.state = 9 if m.state < 7 else 11
        self._since_reset(m.reps[0] + 1)
        self._copy(m.reps[0] + 1, 1)

    def raw_bit(self, cells, index, b):
        """The escape: one decision on any cell of `self.m` (error cases); the plain text and the state are the caller's."""
        self.rc.bit(cells, index, b)

    def raw_direct(self, value, nbits):
        self.rc.direct(value, nbits)

    def expect(self, status):
        """The stream written so far is one the reference answers with `status` (an error the builder cannot see itself)."""
        self.status = status

    # ---- LZMA2 framing ----------------------------------------------------------------------------------------------
    def _l2_rule(self, control, props=None):
        """liblzma's lzma2_decoder.c: the first chunk resets the dictionary; the first LZMA chunk behind a dictionary reset brings
        properties; lc + lp <= 4."""
        if control >= 0xE0 or control == 1:
            self.need_props, self.need_dict_reset = True, False
        elif self.need_dict_reset:
            self._refuse("first chunk without a dictionary reset")
        if control >= 0xC0:
            self.need_props = False
            if props[0] + props[1] > 4:
                self._refuse("lc+lp>4")
        elif control >= 0x80 and self.need_props:
            self._refuse("no properties behind a dictionary-resetting stored chunk" if self.m is not None and control == 0x80 else "no properties")

    def chunk(self, control, props=None):
        assert self.kind == "lzma2" and control in CONTROLS and self.status == 0
        if self.rc is not None:
            self.end_chunk()
        self._l2_rule(control, props)
        self.count["control", control] += 1
        assert not (control == 0x80 and self.end_marked), "behind an end marker rep0 is 0xFFFFFFFF: the next chunk resets the state"
        if control >= 0xC0:
            if self.m is not None and control == 0xC0 and (self.m.lc, self.m.lp, self.m.pb) != tuple(props):
                self.refused.add("property change without a dictionary reset")   # (a construct liblzma's encoder never writes; its decoder takes it)
            self.m = Model(*props)
        elif control == 0xA0:
            if self.m is None:
                self.m = Model(3, 0, 2)      # the reference's defaults
            self.m.reset()
        elif self.m is None:
            self.m = Model(3, 0, 2)          # (cells the decoder does not have: 0x80 first is a trap of the reference -- expect(TRAP))
        if control == 0xE0:
            self.dict_start = self.reset_at = len(self.out)
        self.count["shape", self.m.lc, self.m.lp, self.m.pb] += 1
        self.end_marked = False
        self.rc, self.control, self.chunk_start = RangeEncoder(), control, len(self.out)
        self.props_written = control >= 0xC0

    def end_chunk(self, unpack_delta=0, comp_delta=0, flush_offset=0, props_byte=None):
        """Closes the open chunk: header (control with the high bits of unpack - 1, unpack - 1, comp - 1, properties) and
        payload.  The deltas write deliberately wrong size fields."""
        payload = self.rc.flush(flush_offset)
        unpack = len(self.out) - self.chunk_start + unpack_delta - 1
        comp = len(payload) + comp_delta - 1
        if self.status and unpack_delta == 0:
            unpack += 300            # (the packet that is the error wrote nothing: the field leaves room for what it stood for)
        assert 0 <= unpack < 1 << 21 and 0 <= comp < 1 << 16, (unpack, comp)
        self.stream += bytes([self.control | (unpack >> 16), (unpack >> 8) & 0xFF, unpack & 0xFF, comp >> 8, comp & 0xFF])
        if self.props_written:
            self.stream.append(self.m.props_byte() if props_byte is None else props_byte)
        self.stream += payload
        self.rc = None

    def stored(self, data, reset_dict):
        assert self.kind == "lzma2" and 1 <= len(data) <= 65536 and self.status == 0
        if self.rc is not None:
            self.end_chunk()
        self._l2_rule(1 if reset_dict else 2)
        self.count["control", 1 if reset_dict else 2] += 1
        if reset_dict:
            self.dict_start = self.reset_at = len(self.out)
        n = len(data) - 1
        self.stream += bytes([1 if reset_dict else 2, n >> 8, n & 0xFF]) + bytes(data)
        self._put(bytes(data))

    def raw_bytes(self, data):
        """Bytes between chunks that are no chunk of the builder's (wrong control bytes, garbage)."""
        if self.rc is not None:
            self.end_chunk()
        self.stream += bytes(data)

    # ---- the result -------------------------------------------------------------------------------------------------
    def case(self, name, terminator=True, tail=b"", flush_offset=0):
        if self.kind == "lzma2":
            if self.rc is not None:
                self.end_chunk()
            body = bytes(self.stream) + (b"\0" if terminator else b"")
            props = None
        else:
            body = self.rc.flush(flush_offset)
            props = (self.m.lc, self.m.lp, self.m.pb, self.dict_size, self.declared)
        valid = self.status == 0
        return Case(name, body + tail, self.kind, self.dict_byte, props, bytes(self.out) if valid else None, self.status,
                    len(body) if valid else None, self.ok and valid)


# --------------------------------------------------------------------------------------------------------- random streams
_LENGTHS = [2, 3, 4, 5, 9, 10, 11, 17, 18, 19, 63, 64, 65, 66, 127, 128, 129, 272, 273]
_DISTANCES = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1000, 4095, 4096, 4097, 8191, 65535]


def context_byte(prev, lc):
    """The byte a trained literal coder expects behind `prev`: it depends on exactly the bits that choose the coder."""
    return ((prev >> (8 - lc)) * 167 + 13) & 0xFF if lc else 13


def random_packet(b, rnd, strict, literals=0.45):
    """One legal packet drawn from everything the state allows (strict: only what liblzma decodes too)."""
    pos = len(b.out)
    reach = pos - b.reset_at if strict else pos
    maxd = min(reach, b.dict_size)
    r = rnd.random()
    if r >= literals and not b.window_empty():
        k = rnd.random()
        length = rnd.choice(_LENGTHS) if rnd.random() < 0.3 else rnd.randrange(2, 24)
        if k < 0.45 and maxd >= 1:
            d = rnd.choice(_DISTANCES) if rnd.random() < 0.5 else rnd.randrange(1, maxd + 1)
            if d > maxd:
                d = rnd.randrange(1, maxd + 1)
            return b.match(d, length)
        ok = [i for i in range(4) if b.m.reps[i] + 1 <= reach and not (i == 0 and b.rep0_traps())]
        if k < 0.7 and not b.rep0_traps() and b.m.reps[0] + 1 <= reach:
            return b.short_rep()
        if ok:
            return b.rep(rnd.choice(ok), length)
    k = rnd.random()
    prev = b.out[-1] if pos else 0
    if k < 0.5:
        v = context_byte(prev, b.m.lc)
    elif k < 0.7 and pos > b.m.reps[0]:
        v = b.out[pos - b.m.reps[0] - 1] ^ rnd.choice([0, 0, 1, 0x80, 0x10])
    elif k < 0.85:
        v = (prev + 37) & 0xFF
    else:
        v = rnd.randrange(256)
    b.literal(v)


def random_props(rnd, strict):
    if strict or rnd.random() < 0.4:
        lc = rnd.randrange(5)
        lp = rnd.randrange(5 - lc)
    else:
        lc, lp = rnd.choice([(8, 4), (8, 0), (5, 0), (3, 3), (2, 4), (6, 0), (4, 3), (7, 2), (1, 4), (5, 1)])
    return lc, lp, rnd.choice([0, 1, 2, 2, 3, 4])


def random_stream(rnd, target, strict, counters=None, name="random", constructs=None):
    """A seeded stream of about `target` bytes of output (at least one byte).  strict: only structures that liblzma accepts
    (the Case says liblzma_ok); otherwise everything the reference accepts: lc + lp up to 12, 0x80 / 0xA0 behind a stored chunk
    that reset the dictionary, property changes without a dictionary reset, matches across dictionary resets, end markers inside
    chunks, raw LZMA with a dictionary of a few bytes.  constructs: a set that receives the liblzma-refused constructs (and the
    property changes without a dictionary reset, which liblzma's decoder takes and its encoder never writes) of the stream."""
    b = _random_builder(rnd, target, strict, counters)
    if constructs is not None:
        constructs |= b.refused
    return b.case(name)


def _random_builder(rnd, target, strict, counters):
    if rnd.random() < 0.3:
        small = not strict and rnd.random() < 0.3
        ds = rnd.choice([0, 1, 2, 3, 5, 100]) if small else rnd.choice([4096, 4097, 6000, 1 << 16, 1 << 24])
        how = rnd.randrange(3)   # 0: unknown size + end marker; 1: declared size; 2: declared size + end marker
        b = Builder("lzma", props=random_props(rnd, strict), dict_size=ds, declared=-1, counters=counters)
        while len(b.out) < max(target, 1):
            random_packet(b, rnd, strict)
        if how:
            b.declared = len(b.out)
        if how == 2 and strict:
            how = 1
        if how != 1:
            b.end_marker(rnd.choice([2, 5, 273]))
        return b
    b = Builder("lzma2", dict_byte=rnd.choice([0, 0, 1, 2, 6, 12, 18]), counters=counters)
    while True:
        # a stored chunk now and then, then the next LZMA chunk
        if rnd.random() < (0.3 if b.m is None else 0.25):
            reset = b.need_dict_reset if strict and b.need_dict_reset else rnd.random() < 0.4
            n = rnd.choice([1, 2, 5, 100, 1000])
            b.stored(bytes((rnd.randrange(256) if rnd.random() < 0.3 else (i * 7) & 0xFF) for i in range(n)), reset)
            if len(b.out) >= target and rnd.random() < 0.3:
                break
        if strict:
            controls = [0xE0] if b.need_dict_reset else [0xC0, 0xE0] if b.need_props else [0x80, 0x80, 0xA0, 0xC0, 0xE0]
        else:
            controls = [0xA0, 0xC0, 0xE0] if b.m is None or b.end_marked else [0x80, 0x80, 0xA0, 0xC0, 0xE0]
        control = rnd.choice(controls)
        b.chunk(control, random_props(rnd, strict) if control >= 0xC0 else None)
        for _ in range(rnd.choice([1, 2, 7, 40, 150, 400])):
            random_packet(b, rnd, strict)
        if not strict and rnd.random() < 0.1:
            b.end_marker()
        if len(b.out) >= target:
            break
    return b


# ------------------------------------------------------------------------------------------------------- directed streams
COPY_LENGTHS = [2, 3, 4, 5, 62, 63, 64, 65, 66, 67, 126, 127, 128, 129, 130, 272, 273]
COPY_DISTANCES = list(range(1, 67)) + [127, 128, 129, 272, 273, 274, 4095]
SHAPES = [(8, 4, 4), (8, 0, 0), (5, 0, 2), (3, 3, 1), (2, 4, 3), (6, 0, 2), (4, 3, 4)]
STATE_PATHS = {0: "LLL", 1: "LLLMLL", 2: "LLLRLL", 3: "LLLSLL", 4: "LLLML", 5: "LLLRL", 6: "LLLSL", 7: "LLLM", 8: "LLLR", 9: "LLLS",
               10: "LLLMM", 11: "LLLMR"}
FAR_DICT_BYTE = 18     # 2 MiB
FAR_LIMIT = (1 << 21) - 600


def _new(kind, props, counters, dict_byte=12, dict_size=1 << 16, declared=-1):
    """A stream of either kind with its first chunk open."""
    if kind == "lzma":
        return Builder("lzma", props=props, dict_size=dict_size, declared=declared, counters=counters)
    b = Builder("lzma2", dict_byte=dict_byte, counters=counters)
    b.chunk(0xE0, props)
    return b


def _end(b, name):
    """Raw LZMA of unknown size ends with the marker."""
    if b.kind == "lzma" and b.declared < 0 and b.status == 0 and not b.end_marked:
        b.end_marker()
    return b.case(name)


def _trained_literal(b, rnd):
    prev = b.out[-1] if b.out else 0
    b.literal(context_byte(prev, b.m.lc) if rnd.random() < 0.75 else rnd.randrange(256))


def _steer(b):
    """Away from (state 11, pos_state 15): a rep1 keeps state 11 and moves the position."""
    while b.rep0_traps():
        b.rep(1, 3)


def _state_machine(kind, pb, counters):
    rnd = random.Random(0x57A7E + pb)
    b = _new(kind, (3, 1, pb), counters)
    for _ in range(40):
        b.literal(rnd.randrange(256))
    for d, n in ((7, 3), (13, 4), (21, 5), (30, 6)):
        b.match(d, n)
    for state in range(12):
        for k in KINDS:
            for step in STATE_PATHS[state]:
                if step == "L":
                    b.literal(rnd.randrange(256))
                elif step == "M":
                    b.match(rnd.randrange(1, 40), rnd.randrange(2, 20))
                elif step == "R":
                    b.rep(rnd.randrange(1, 4), rnd.randrange(2, 20))
                else:
                    _steer(b)
                    b.short_rep()
            assert b.m.state == state
            if k in ("rep0", "shortrep"):
                _steer(b)
                assert b.m.state == state
            if k == "literal":
                b.literal(rnd.randrange(256))
            elif k == "match":
                b.match(rnd.randrange(1, 40), rnd.choice([2, 9, 18, 70]))
            elif k == "shortrep":
                b.short_rep()
            else:
                b.rep(int(k[3]), rnd.choice([2, 3, 9, 18, 70]))
    return _end(b, "states-x-packets-pb%d-%s" % (pb, kind))


def _trap_point(short, counters):
    b = _new("lzma2", (3, 0, 4), counters)
    for i in range(27):
        b.literal(65 + i)
    b.match(3, 2)
    b.rep(1, 2)
    assert b.m.state == 11 and b.pos_state() == 15
    b.short_rep() if short else b.rep(0, 5)
    assert b.status == TRAP
    return b.case("state-11-pos-state-15-%s-rep0-traps" % ("short" if short else "long"))


def _copy_shapes(lc, half, through_reps, counters):
    rnd = random.Random(0xC0B1 + lc * 4 + half * 2 + through_reps)
    b = _new("lzma2", (lc, 0, 2), counters, dict_byte=0)
    for _ in range(300):
        _trained_literal(b, rnd)
    cut = len(COPY_DISTANCES) // 2
    for d in (COPY_DISTANCES[:cut] if half == 0 else COPY_DISTANCES[cut:]):
        if through_reps:
            b.match(d, 2)
            _trained_literal(b, rnd)
        for n in COPY_LENGTHS:
            if through_reps:
                _steer(b)
                b.rep(0, n)
            else:
                b.match(d, n)
            _trained_literal(b, rnd)      # the literal right behind the copy: its coder is chosen by the copy's last byte
    assert len(b.out) <= 65536
    return b.case("copy-shapes-lc%d-distances-%s-%s" % (lc, "1-to-35" if half == 0 else "36-to-4095", "reps" if through_reps else "matches"))


def _every_length(pb, through_reps, counters):
    rnd = random.Random(0x1E46 + pb * 2 + through_reps)
    b = _new("lzma2", (3, 0, pb), counters)
    for _ in range(64):
        b.literal(rnd.randrange(256))
    b.match(17, 4), b.match(33, 4), b.match(49, 4), b.match(60, 4)
    for n in range(2, 274):
        if through_reps:
            i = n % 4
            if i == 0:
                _steer(b)
            b.rep(i, n)
        else:
            b.match(rnd.randrange(1, 64), n)
        b.literal(rnd.randrange(256))
    for ps in range(1 << pb):             # the low and mid trees of every pos_state
        for n in (2, 9, 10, 17, 18):
            while b.pos_state() != ps:
                b.literal(rnd.randrange(256))
            if through_reps:
                b.rep(1, n)
            else:
                b.match(rnd.randrange(1, 64), n)
    assert len(b.out) <= 65536
    return b.case("every-length-%s-pb%d" % ("rep-coder" if through_reps else "length-coder", pb))


def slot_patterns(slot):
    """The extra bits of a pos slot: all zero, all one, alternating both ways."""
    if slot < 4:
        return [0]
    ndb = (slot >> 1) - 1
    ones = (1 << ndb) - 1
    return sorted({0, ones, 0xAAAAAAAA & ones, 0x55555555 & ones})


def _every_slot_far(counters):
    """Every pos slot that 2 MiB of output allow (0 .. 41), each with its extra bits all zero, all one and alternating; the output
    between them is made of length-273 matches (and a literal each, so that it never becomes periodic)."""
    rnd = random.Random(0xFA2)
    b = _new("lzma2", (3, 0, 2), counters, dict_byte=FAR_DICT_BYTE)
    for _ in range(64):
        b.literal(rnd.randrange(256))
    for slot in range(42):
        for rem in slot_patterns(slot):
            d = slot_base(slot) + rem + 1
            if d > FAR_LIMIT:
                continue
            while len(b.out) < d:
                b.match(rnd.randrange(1, min(len(b.out), 3000) + 1), 273)
                b.literal(rnd.randrange(256))
            b.match(d, rnd.choice([2, 3, 4, 5, 64]))
            b.literal(rnd.randrange(256))
    assert len(b.out) <= 1 << 21
    return b.case("every-pos-slot-to-2MiB")


def _slot_error(slot, rem, counters, name):
    b = _new("lzma2", (3, 0, 2), counters, dict_byte=39)   # the largest dictionary of the format: 3 << 30
    for i in range(20):
        b.literal(i)
    b.match(slot_base(slot) + rem + 1, 4)
    assert b.status == NOT_ENOUGH
    return b.case(name)


def _limits(kind, counters):
    """One decision several hundred times, then its opposite: a cell in LDS (isMatch), literal cells, a `high` length cell."""
    b = _new(kind, (3, 0, 0), counters)
    for _ in range(400):
        b.literal(0)                      # isMatch[0] and the literal cells of coder 0 go to 2017
    b.literal(0xFF)                       # ... and the other way on the saturated literal cells
    b.literal(0)
    for _ in range(300):
        b.match(2, 19)                    # `high` symbol 1: the root of the tree goes to 2017, the last cell of the path to 31
    b.match(2, 18 + 0x80)                 # ... and the root the other way
    b.match(2, 18)                        # ... and the last cell
    b.literal(7)
    for _ in range(300):
        b.rep(0, 19)
    b.rep(0, 273)
    b.rep(0, 18)
    b.literal(9)
    return _end(b, "probabilities-at-their-limits-" + kind)


def _model_shape(kind, shape, counters):
    """Several thousand symbols under one model shape; the previous bytes walk through more literal coders than four cache
    lines hold (and come back to them: the lines are written back and reloaded with their adapted cells)."""
    lc, lp, pb = shape
    rnd = random.Random(0x5A9E + lc * 100 + lp * 10 + pb)
    b = _new(kind, shape, counters)
    for i in range(3000):
        if kind == "lzma2" and i in (1000, 2000):
            b.chunk(0x80 if i == 1000 else 0xA0)
        if i % 3 == 0 and not b.window_empty():
            random_packet(b, rnd, False, literals=0.2)
        else:
            prev = b.out[-1] if b.out else 0
            b.literal(((prev + 37) & 0xFF) if rnd.random() < 0.8 else context_byte(prev, lc))
    return _end(b, "model-lc%d-lp%d-pb%d-%s" % (lc, lp, pb, kind))


def _property_changes(shapes, reset_dict, counters, name):
    rnd = random.Random(0x9209 + len(name) + reset_dict)
    b = Builder("lzma2", dict_byte=6, counters=counters)
    for k, shape in enumerate(shapes):
        b.chunk(0xE0 if k == 0 or reset_dict else 0xC0, shape)
        for _ in range(700):
            random_packet(b, rnd, reset_dict)
    return b.case(name)


def _state_reset_after_adapted_cells(counters):
    rnd = random.Random(0xA0)
    b = _new("lzma2", (3, 0, 2), counters)
    for _ in range(1500):
        random_packet(b, rnd, True)
    b.chunk(0xA0)                         # every cell 1,024 again, reps 0, state 0 -- the dictionary stays
    for _ in range(1500):
        random_packet(b, rnd, True)
    return b.case("state-reset-0xA0-after-adapted-cells")


def _continue_behind_stored(reset_dict, counters):
    rnd = random.Random(0x80 + reset_dict)
    b = _new("lzma2", (4, 0, 2), counters)
    for _ in range(200):
        _trained_literal(b, rnd)
    b.match(5, 7)                         # state 7, rep0 4: the next literal is a matched one
    b.stored(bytes([0xF3, 0x5A, 0xC4, 0x3D, 0xE1, 0x96, 0x0F, 0x78, 0xB2]), reset_dict)
    b.chunk(0x80)
    b.literal(0xE1 ^ 0x04)                # matched against the stored 0xE1 (rep0 4), in the coder chosen by the stored 0xB2
    b.match(7, 12)                        # source: stored bytes, overlapping
    _trained_literal(b, rnd)
    b.rep(1, 3)
    for _ in range(200):
        random_packet(b, rnd, False)
    return b.case("0x80-behind-a-stored-chunk" + ("-that-reset-the-dictionary" if reset_dict else ""))


def _many_dictionary_resets(counters):
    """0xE0 in mid-stream, 64 times: the literal behind each reset has context 0 whatever the last byte before it was."""
    rnd = random.Random(0xE0E0)
    b = Builder("lzma2", dict_byte=0, counters=counters)
    for k in range(64):
        b.chunk(0xE0, (3, 0, 2))
        for i in range(12):
            b.literal(0x10 | (i & 7))     # context 0
        b.short_rep()
        b.match(3, 4)
        b.literal(0xE0 | rnd.randrange(32))   # the last byte before the reset: its top bits are all ones
    return b.case("dictionary-reset-0xE0-mid-stream-64-times")


def _stored_reset_mid_stream(counters):
    rnd = random.Random(0x01)
    b = _new("lzma2", (3, 0, 2), counters)
    for _ in range(300):
        random_packet(b, rnd, True)
    b.stored(b"\xFF" * 5, True)
    b.chunk(0x80)                         # the model goes on: state, reps and cells as they were
    b.rep(0, 3) if not b.rep0_traps() else b.rep(1, 3)   # legal: the window holds the stored bytes
    for _ in range(300):
        random_packet(b, rnd, False)
    return b.case("dictionary-reset-0x01-mid-stream-then-0x80")


def _rep_first_after_reset(short, counters):
    b = _new("lzma2", (3, 0, 2), counters)
    for i in range(50):
        b.literal(i)
    b.match(9, 5)
    b.chunk(0xE0, (3, 0, 2))
    b.short_rep() if short else b.rep(0, 4)
    assert b.status == WINDOW_EMPTY
    return b.case("%s-rep-first-behind-a-dictionary-reset" % ("short" if short else "long"))


def _match_behind_reset(counters):
    b = _new("lzma2", (3, 0, 2), counters)
    for i in range(100):
        b.literal((i * 3) & 0xFF)
    b.chunk(0xE0, (3, 0, 2))
    b.literal(1)
    b.match(60, 30)                       # source: before the reset.  The reference checks the output, not the window
    b.literal(2)
    return b.case("match-reaching-behind-a-dictionary-reset")


def _sliding_window(how, counters):
    rnd = random.Random(0x511DE + len(how))
    b = _new("lzma2", (3, 0, 2), counters, dict_byte=0)
    if how == "literals":
        for _ in range(5000):
            _trained_literal(b, rnd)
    elif how == "matches":
        for _ in range(100):
            b.literal(rnd.randrange(256))
        while len(b.out) < 9000:
            b.match(rnd.randrange(1, min(len(b.out), 4096) + 1), rnd.choice([2, 64, 200, 273]))
            b.literal(rnd.randrange(256))
    else:
        b.literal(5)
        b.stored(bytes(rnd.randrange(256) for _ in range(4090)), False)    # 4,091 bytes: the window is not full yet
        b.stored(bytes(rnd.randrange(256) for _ in range(5)), False)       # exactly full
        b.stored(bytes(rnd.randrange(256) for _ in range(3000)), False)
        b.chunk(0x80)
    b.match(4096, 40)                     # the farthest byte of the slid window
    for _ in range(200):
        random_packet(b, rnd, True)
    return b.case("4KiB-window-sliding-under-" + how)


def _dictionary_edge(beyond, counters):
    rnd = random.Random(0xED6E)
    b = _new("lzma2", (3, 0, 2), counters, dict_byte=0)
    while len(b.out) < 4200:
        b.literal(rnd.randrange(256))
        b.match(rnd.randrange(1, min(len(b.out), 4096) + 1), 60)
    b.match(4097 if beyond else 4096, 9)
    assert b.status == (NOT_ENOUGH if beyond else 0)
    if not beyond:
        b.literal(3)
    return b.case("distance-dict-size" + ("-plus-one" if beyond else ""))


def _tiny_dictionary(ds, declared, counters):
    """Raw LZMA with a dictionary of 0 .. 3 bytes.  0: the window never slides (dict_start stays 0) and no match is legal, reps
    are; 1: the window is always empty -- every literal has context 0 and a rep is windowIsEmpty; 2, 3: matches up to that distance."""
    rnd = random.Random(0x7197 + ds)
    b = Builder("lzma", props=(4, 0, 2), dict_size=ds, counters=counters)
    for i in range(600):
        k = rnd.random()
        if ds == 1 or b.window_empty() or k < 0.5:
            _trained_literal(b, rnd)
        elif k < 0.65:
            b.short_rep()
        elif k < 0.85 or ds < 2:
            b.rep(0, rnd.choice([2, 3, 10, 70]))
        else:
            b.match(rnd.randrange(1, min(ds, len(b.out)) + 1), rnd.choice([2, 5, 66]))
    if declared:
        b.declared = len(b.out)
    return _end(b, "raw-lzma-dictionary-of-%d-bytes-%s" % (ds, "declared-size" if declared else "end-marker"))


def _tiny_dictionary_errors(counters):
    out = []
    b = Builder("lzma", props=(3, 0, 2), dict_size=1, counters=counters)
    b.literal(1), b.literal(2)
    b.short_rep()
    assert b.status == WINDOW_EMPTY
    out.append(b.case("raw-lzma-dictionary-of-1-byte-rep-is-window-empty"))
    b = Builder("lzma", props=(3, 0, 2), dict_size=0, counters=counters)
    b.literal(1), b.literal(2)
    b.match(1, 2)
    assert b.status == NOT_ENOUGH
    out.append(b.case("raw-lzma-dictionary-of-0-bytes-match-is-not-enough-to-repeat"))
    return out


def _ends(counters):
    out = []
    rnd = random.Random(0xE2D)

    def chunk_of(n=120):
        b = _new("lzma2", (3, 0, 2), counters)
        for _ in range(n):
            random_packet(b, rnd, True)
        return b

    b = chunk_of()
    b.end_marker()
    out.append(b.case("end-marker-at-exactly-unpack"))
    b = chunk_of()
    b.end_marker()
    b.end_chunk(unpack_delta=3)
    b.expect(WRONG_SIZES)
    out.append(b.case("end-marker-before-unpack"))
    for marker in (False, True):
        b = Builder("lzma", props=(3, 0, 2), dict_size=1 << 16, counters=counters)
        for _ in range(300):
            random_packet(b, rnd, True)
        b.declared = len(b.out)
        if marker:
            b.end_marker()
        out.append(b.case("raw-lzma-declared-size" + ("-then-end-marker" if marker else "")))
    b = Builder("lzma", props=(3, 0, 2), dict_size=1 << 16, counters=counters)
    for _ in range(300):
        random_packet(b, rnd, True)
    b.end_marker(273)
    out.append(b.case("raw-lzma-unknown-size-end-marker"))
    # the declared size reached with code != 0 and no marker behind it: the decoder goes on into the flush bytes
    b = Builder("lzma", props=(3, 0, 2), dict_size=1 << 16, counters=counters)
    for i in range(40):
        b.literal(i)
    b.declared = 30
    b.expect(EXCEEDED)
    out.append(b.case("raw-lzma-declared-size-reached-with-code-not-zero"))
    # end marker, then a range coder that is not finished: rangeDecoderFinishError
    b = Builder("lzma", props=(3, 0, 2), dict_size=1 << 16, counters=counters)
    for i in range(40):
        b.literal(i)
    b.end_marker()
    b.expect(FINISH_ERROR)
    out.append(b.case("raw-lzma-end-marker-with-code-not-zero", flush_offset=0x40))
    # the size fields of a chunk, off by one each way
    # (unpack + 1: the decoder goes on behind the flush -- code 0 decodes as a literal 0 -- and then finds a packet more than the size)
    for field, delta, status in (("unpack", 1, EXCEEDED), ("unpack", -1, EXCEEDED), ("comp", 1, WRONG_SIZES), ("comp", -1, WRONG_SIZES)):
        b = chunk_of(60)
        b.literal(0x55)
        b.end_chunk(**{field + "_delta": delta})
        b.chunk(0x80)
        b.literal(0x66)
        b.expect(status)
        out.append(b.case("chunk-%s-field-%s-one" % (field, "plus" if delta > 0 else "minus")))
    b = chunk_of(60)
    b.match(5, 10)
    b.end_chunk(unpack_delta=-3)
    b.expect(WILL_EXCEED)
    out.append(b.case("repeat-will-exceed-unpack"))
    for site in ("literal", "rep", "match"):   # the three sites of exceededUncompressedSize: one packet more than unpack says
        b = chunk_of(60)
        if site == "literal":
            b.literal(0x41)
        elif site == "rep":
            b.rep(1, 2)
        else:
            b.match(3, 2)
        b.end_chunk(unpack_delta=-(1 if site == "literal" else 2))
        b.expect(EXCEEDED)
        out.append(b.case("exceeded-uncompressed-size-at-a-" + site))
    return out


def _framing_errors(counters):
    out = []
    b = Builder("lzma2", dict_byte=12, counters=counters)
    b.chunk(0x80)
    b.literal(1)
    b.expect(TRAP)
    out.append(b.case("0x80-first-has-no-model"))
    b = Builder("lzma2", dict_byte=12, counters=counters)
    b.chunk(0xA0)                         # legal for the reference: the default properties
    for i in range(100):
        b.literal((i * 5) & 0xFF)
    b.match(10, 20)
    out.append(b.case("0xA0-first-uses-the-default-properties"))
    b = _new("lzma2", (3, 0, 2), counters)
    b.literal(1)
    b.raw_bytes(b"\x03\x00\x00\x00")
    b.expect(WRONG_CONTROL)
    out.append(b.case("control-byte-3"))
    b = _new("lzma2", (3, 0, 2), counters)
    b.literal(1)
    b.end_chunk(props_byte=225)
    b.expect(WRONG_PROPERTIES)
    out.append(b.case("properties-byte-225"))
    b = _new("lzma2", (3, 0, 2), counters, dict_byte=40)
    b.literal(1)
    b.expect(WRONG_DICT)
    out.append(b.case("dictionary-byte-40"))
    b = _new("lzma2", (3, 0, 2), counters)
    for i in range(30):
        b.literal(i)
    out.append(b.case("garbage-behind-the-terminator", tail=b"\xE0\x12\x34"))
    return out


def _input_window(counters):
    """The decoder keeps 256 input bytes in a register and refills it at one place per symbol (and per chunk) when fewer than 48
    are left: stream lengths of every residue mod 4, a chunk header starting at each of the last eight offsets that are read
    WITHOUT a refill (201 .. 208), and every one of these cut short by 1 .. 8 bytes."""
    out = []
    whole = []
    for residue in range(4):
        n = 300
        while True:
            rnd = random.Random(0x19 + residue)
            b = _new("lzma2", (3, 0, 2), counters)
            for _ in range(n):
                random_packet(b, rnd, True, literals=0.8)
            c = b.case("stream-length-%d-mod-4" % residue)
            if len(c.stream) % 4 == residue:
                break
            n += 1
        whole.append(c)
    for k in range(8):
        rnd = random.Random(0x1900 + k)
        b = Builder("lzma2", dict_byte=12, counters=counters)
        b.stored(bytes(rnd.randrange(256) for _ in range(198 + k)), True)
        assert len(b.stream) == 201 + k
        b.chunk(0xE0, (3, 0, 2))
        for _ in range(150):
            random_packet(b, rnd, True, literals=0.8)
        b.chunk(0x80)
        for _ in range(150):
            random_packet(b, rnd, True, literals=0.8)
        whole.append(b.case("chunk-header-at-window-offset-%d" % (201 + k)))
    out += whole
    for c in whole:
        for cut in range(1, 9):           # the terminator, then the flush bytes of the last chunk: a read past the end of the input
            out.append(Case("%s-cut-by-%d" % (c.name, cut), c.stream[:-cut], "lzma2", c.dict_byte, None, None, TRAP, None, False))
    return out


def _build_directed(counters):
    cases = []
    for pb in (0, 2, 4):
        cases.append(_state_machine("lzma2", pb, counters))
    cases.append(_state_machine("lzma", 4, counters))
    cases += [_trap_point(False, counters), _trap_point(True, counters)]
    for lc in (4, 8):
        for through_reps in (0, 1):
            for half in (0, 1):
                cases.append(_copy_shapes(lc, half, through_reps, counters))
    for pb in (0, 2, 4):
        for through_reps in (0, 1):
            cases.append(_every_length(pb, through_reps, counters))
    cases.append(_every_slot_far(counters))
    for slot in (42, 47, 55, 62):
        cases.append(_slot_error(slot, slot_patterns(slot)[1], counters, "pos-slot-%d-is-not-enough-to-repeat" % slot))
    cases.append(_slot_error(63, (1 << 30) - 2, counters, "largest-distance-is-not-enough-to-repeat"))
    cases += [_limits("lzma2", counters), _limits("lzma", counters)]
    for shape in SHAPES:
        cases += [_model_shape("lzma2", shape, counters), _model_shape("lzma", shape, counters)]
    for reset_dict in (0, 1):
        suffix = "-with-dictionary-resets" if reset_dict else ""
        cases.append(_property_changes([(4, 0, 2), (0, 0, 0), (0, 4, 4)], reset_dict, counters, "properties-4-to-0-to-4" + suffix))
        cases.append(_property_changes([(3, 0, 2), (8, 4, 4), (3, 0, 2)], reset_dict, counters, "properties-3-to-12-to-3" + suffix))
    cases.append(_state_reset_after_adapted_cells(counters))
    cases += [_continue_behind_stored(False, counters), _continue_behind_stored(True, counters)]
    cases += [_many_dictionary_resets(counters), _stored_reset_mid_stream(counters)]
    cases += [_rep_first_after_reset(False, counters), _rep_first_after_reset(True, counters), _match_behind_reset(counters)]
    cases += [_sliding_window(how, counters) for how in ("literals", "matches", "stored-chunks")]
    cases += [_dictionary_edge(False, counters), _dictionary_edge(True, counters)]
    for ds in range(4):
        cases += [_tiny_dictionary(ds, False, counters), _tiny_dictionary(ds, True, counters)]
    cases += _tiny_dictionary_errors(counters)
    cases += _ends(counters)
    cases += _framing_errors(counters)
    cases += _input_window(counters)
    assert len({c.name for c in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def _directed():
    counters = collections.Counter()
    return tuple(_build_directed(counters)), counters


def directed_cases():
    """The named corners, built once per process."""
    return list(_directed()[0])


def directed_counters():
    """What the directed set wrote: ("packet", kind, state), ("slot", s), ("len", coder, tier), ("len-value", coder, length),
    ("control", byte), ("shape", lc, lp, pb), ("coder", literal coder)."""
    return _directed()[1]
