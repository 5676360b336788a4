"""Deflate streams around PAIR table entries (csrc/inflate_sync.h: a length code, its extra bits and the distance code behind it
in one direct entry), built code by code with _deflate_build.  TEST INFRASTRUCTURE; standard library only.

Every stream starts with a stored block of text, so that matches have something to copy, then one or more dynamic blocks over
code sets short enough for most matches to pair (lengths 3 .. 10 and 11 .. 22 at 3 .. 5 bits, distances at 2 .. 4 bits).  The
first round of a block starts at the byte, rounded down to four, in which the header ends; sub-chunk k of it ends 68 k bytes
further on (kSyncChunk).  `directed()` gives (name, stream, cap or None): expectations come from the oracle."""
import functools
import random

import _deflate_build as B

CHUNK = 68
E_TRAP, E_CAPACITY, E_NOT_FOUND = 900, 901, 104


def fill_complete(lengths, fillers):
    """{symbol: length} made complete: the space left is given to `fillers` in turn, one code per set bit of it."""
    d = dict(lengths)
    left = (1 << 15) - sum(1 << (15 - l) for l in d.values())
    assert left >= 0
    fillers = list(fillers)
    for bit in range(14, -1, -1):
        if left >> bit & 1:
            d[fillers.pop(0)] = 15 - bit
    assert B.is_complete(d.values())
    return d


# literals a / b at 3 / 4 bits (any bit position can be reached with them), the lengths that pair, end of block at 6 bits
LIT = fill_complete({97: 3, 98: 4, 257: 3, 258: 4, 264: 4, 265: 4, 269: 5, 285: 5, 256: 6, 273: 6}, [120, 121, 122, 123, 124])
DIST = fill_complete({0: 2, 1: 2, 4: 3, 29: 3}, [2, 3, 5, 6])
LIT_V, DIST_V = B.vector(LIT, 286), B.vector(DIST, 30)
PAIR = ("sym", 258, 0, 4, 1)            # length 4, distance 6: 4 + 3 + 1 bits, one direct entry
LONG_PAIR = ("sym", 269, 2, 29, 8191)   # length 21, distance 32768: 5 + 2 + 3 index bits, 13 extra bits behind them
MATCH = ("sym", 257, 0, 0, 0)           # length 3, distance 1 (a pair as well)
TEXT = B._text(random.Random(0x9A125), 40000)


class Stream:
    def __init__(self, prefix=300, lit=None, dist=None):
        self.w = B.BitWriter()
        self.n_out = 0
        self.since_match = 0
        self.lit_v, self.dist_v = lit or LIT_V, dist or DIST_V
        if prefix:
            B.stored_block(self.w, TEXT[:prefix], False)
            self.n_out = prefix
        self.round_base = None

    def header(self, final=True):
        B.dynamic_block(self.w, [], final, self.lit_v, self.dist_v, eob=False)
        self.lc, self.dc = B._reversed_codes(self.lit_v), B._reversed_codes(self.dist_v)
        self.round_base = 8 * ((self.w.bit_length() >> 3) & ~3)
        self.since_match = 0

    def boundary(self, k):
        """The bit at which sub-chunk k - 1 of the block's first round ends."""
        return self.round_base + 8 * CHUNK * k

    def put(self, *tokens):
        for t in B.normalise(tokens):
            B._write_tokens(self.w, [t], self.lc, self.dc, False)
            if isinstance(t, int):
                self.n_out += 1
                self.since_match += 1
            elif t[0] == "sym":
                self.n_out += B.LEN_BASE[t[1] - 257] + t[2]
                self.since_match = 0

    def pad_to(self, target):
        """Literals of 3 and 4 bits, a short match at least every 60 of them, until the next code starts at bit `target`."""
        assert target - self.w.bit_length() >= 6
        while target - self.w.bit_length() > 300:
            self.put(*([97, 98, 97] * 13), MATCH)
        r = target - self.w.bit_length()
        if self.since_match + r // 3 > 100 and r > 30:
            self.put(MATCH)
            r = target - self.w.bit_length()
        y = next(y for y in range(3) if (r - 4 * y) % 3 == 0 and r >= 4 * y)
        self.put(*([98] * y + [97] * ((r - 4 * y) // 3)))
        assert self.w.bit_length() == target

    def eob(self):
        B._write_tokens(self.w, [], self.lc, self.dc, True)

    def data(self, cut=None):
        d = self.w.data()
        return d if cut is None else d[:cut]


def linked_runs():
    """name -> units (_deflate_linked_cases.U): an open unit of five literals, then a linked unit (SWC_DEFLATE_JOINED |
    SWC_DEFLATE_LINKED) whose first symbol is a pair that reaches exactly to the first byte of its history, and one beyond it."""
    import _deflate_linked_cases as L
    runs = {}
    for name, distance in (("exactly-into", 5), ("one-beyond", 6)):
        head = Stream(prefix=0)
        head.header(final=False)
        head.put(97, 98, 120, 97, 98)
        head.eob()
        B.stored_block(head.w, b"", False)          # the sync flush the stream is cut at
        unit = Stream(prefix=0)
        unit.n_out = 5
        unit.header()
        unit.put(("sym", 258, 0) + B._DIST_SYM[distance], 98, PAIR)
        unit.eob()
        runs["linked-pair-reaches-%s-its-history" % name] = [L.U(head.data(), 5, L.OPEN, True), L.U(unit.data(), 9, L.JL, False)]
    return runs


def _code_bits(s, sym):
    return s.lit_v[sym]


@functools.lru_cache(maxsize=None)
def directed():
    out = []

    # a pair whose length code ends one bit in front of, at and one bit behind the end of a sub-chunk
    for k in (1, 2, 63, 64):
        for delta in (-1, 0, 1):
            for tok, name in ((PAIR, "pair"), (LONG_PAIR, "long-pair")):
                if tok is LONG_PAIR and k not in (1, 64):
                    continue
                s = Stream(prefix=33000 if tok is LONG_PAIR else 300)
                s.header()
                s.pad_to(s.boundary(k) + delta - _code_bits(s, tok[1]))
                s.put(tok, *([97, 98] * 15), tok, 97)
                s.eob()
                out.append(("%s-length-code-ends-%+d-at-boundary-%d" % (name, delta, k), s.data(), None))

    # the last symbol of a block; the first symbol of a block behind literals that no record covers yet
    s = Stream()
    s.header(final=False)
    s.put(*([97] * 10))
    s.eob()
    s.header(final=False)
    s.put(PAIR, 98, 98, PAIR)
    s.eob()
    s.header()
    s.put(PAIR)
    s.eob()
    out.append(("pair-first-behind-pending-literals-and-last-of-block", s.data(), None))

    # a distance one beyond the output, and exactly the output, at positions 0, 1 and 32,767
    for at in (0, 1, 32767):
        for over in (1, 0):
            if at == 0 and over == 0:
                continue
            s = Stream(prefix=at if at > 1 else 0)
            s.header()
            if at == 1:
                s.put(97)
            s.put(("sym", 258, 0) + B._DIST_SYM[at + over], 98)
            s.eob()
            out.append(("pair-distance-%s-the-output-at-%d" % ("one-beyond" if over else "exactly", at), s.data(), None))

    # the input ends behind the length code, inside the distance code, inside the distance's extra bits
    for name, back in (("behind-the-length-code", 0), ("inside-the-distance-code", 1), ("inside-the-distance-extra-bits", 4)):
        s = Stream(prefix=33000)
        s.header()
        t = (s.w.bit_length() + 2000) & ~7
        s.pad_to(t - back - (_code_bits(s, 269) + 2))
        s.put(LONG_PAIR, 97, 97)
        s.eob()
        out.append(("input-ends-" + name, s.data(cut=t // 8), None))

    # the capacity ends inside a pair's length
    s = Stream()
    s.header()
    s.put(*([97, 98] * 20))
    before = s.n_out
    s.put(("sym", 264, 0, 4, 0), 97, PAIR)
    s.eob()
    for inside in (1, 9):
        out.append(("capacity-%d-bytes-into-a-pair" % inside, s.data(), before + inside))
    s = Stream()
    s.header()
    s.pad_to(s.boundary(70) + 1)
    before = s.n_out
    s.put(("sym", 264, 0, 4, 0), 97, PAIR)
    s.eob()
    out.append(("capacity-inside-a-pair-in-the-second-round", s.data(), before + 5))

    # more literals in front of a pair than one record carries
    s = Stream()
    s.header()
    s.put(*([97, 98, 120] * 70), PAIR, *([98] * 130), PAIR, 97)
    s.eob()
    out.append(("more-than-127-literals-in-front-of-a-pair", s.data(), None))

    # pairs only: 4,096 matches of length 3 .. 10 at distance 1 .. 4
    rnd = random.Random(4096)
    lit = fill_complete({257: 3, 258: 3, 259: 3, 260: 3, 261: 4, 262: 4, 263: 4, 264: 4, 97: 4, 256: 5}, [98, 99, 100])
    dist = {0: 2, 1: 2, 2: 2, 3: 2}
    s = Stream(prefix=0, lit=B.vector(lit, 286), dist=B.vector(dist, 30))
    s.header()
    s.put(97, 97, 97, 97)
    for _ in range(4096):
        s.put((rnd.randrange(3, 11), rnd.randrange(1, 5)))
    s.eob()
    out.append(("4096-pairs-and-nothing-else", s.data(), None))

    # no pair at all: stored, fixed, literals only
    w = B.BitWriter()
    B.stored_block(w, TEXT[:5000], True)
    out.append(("stored-only", w.data(), None))
    w = B.BitWriter()
    B.stored_block(w, TEXT[:100], False)
    tokens, _ = B._random_tokens(random.Random(5), 1, 100, 9000)
    B.fixed_block(w, tokens, True)
    out.append(("fixed-codes-pair-nowhere", w.data(), None))
    s = Stream(prefix=0)
    s.header()
    s.put(*[rnd.choice([97, 98, 120, 121, 122]) for _ in range(9000)])
    s.eob()
    out.append(("literals-only", s.data(), None))

    assert len({n for n, _, _ in out}) == len(out)
    return tuple(out)
