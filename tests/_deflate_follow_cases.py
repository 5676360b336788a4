"""Deflate streams around the FOLLOW-UP LITERAL of the provisional decode (csrc/inflate_sync.h, decode_chunk_prov: a step takes the
plain literal behind its own code as well), built code by code with _deflate_build, and a model of the steps a lane then takes.
TEST INFRASTRUCTURE; standard library only.

Every stream is one dynamic block (a stored block of text in front of it where matches need something to copy) that ends inside
the block's first round: sub-chunk k of it ends at `boundary(k + 1)`, a code belongs to the lane whose sub-chunk it starts in, and
lane 0 starts at the block's first code.  `Logged` notes every code it writes: (first bit, bits, kind), kind one of
lit / long (a literal whose code is longer than the table index) / pair / len / dist / eob / bad."""
import functools
import random

import _deflate_build as B
import _deflate_pairs_cases as PC

LIT_BITS, PAIR_LEN_MAX, CHUNK = 10, 127, PC.CHUNK
HELD_MAX = 64 - (LIT_BITS + 2)      # form (b): offset in the held window + the step's bits may be this at the most

# the pairing set of _deflate_pairs_cases (literals a / b / x at 3 / 4 / 2 bits); 285 (length 258) never pairs
NOPAIR = ("sym", 285, 0, 0, 0)      # length 258 at distance 1: a length step, then a distance step
BIGPAIR = PC.LONG_PAIR              # 5 + 2 + 3 + 13 = 23 bits: the largest pair there is
# a set with literals behind links (A, B, C: 11, 12, 12 bits) and a code of exactly 10 bits
DEEP = {97: 3, 98: 4, 257: 3, 258: 4, 264: 4, 285: 5, 256: 6, 120: 2, 121: 3, 122: 3, 123: 7, 124: 8, 125: 9, 126: 10, 65: 11, 66: 12, 67: 12}
assert B.is_complete(DEEP.values())
DEEP_V = B.vector(DEEP, 286)


class Logged(PC.Stream):
    def __init__(self, prefix=300, lit=None, dist=None):
        super().__init__(prefix, lit, dist)
        self.codes = []

    def put(self, *tokens):
        for t in B.normalise(tokens):
            at = self.w.bit_length()
            if isinstance(t, int):
                n = self.lit_v[t]
                self.codes.append((at, n, "lit" if n <= LIT_BITS else "long"))
            elif t[0] == "sym":
                nl = self.lit_v[t[1]] + B.LEN_BITS[t[1] - 257]
                dn = self.dist_v[t[3]]
                nd = dn + B.DIST_BITS[t[3]]
                if nl + dn <= LIT_BITS and B.LEN_BASE[t[1] - 257] + t[2] <= PAIR_LEN_MAX:
                    self.codes.append((at, nl + nd, "pair"))
                else:
                    self.codes += [(at, nl, "len"), (at + nl, nd, "dist")]
            else:
                assert t[0] == "code" and t[1] == "lit" and t[2] > 285
                self.codes.append((at, self.lit_v[t[2]], "bad"))
            super().put(t)

    def fixed_header(self, final=True):
        """A block of the fixed codes (286 and 287 have codes there, and no match pairs: a length takes 7 bits, a distance 5)."""
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        self.lit_v, self.dist_v = B.FIXED_LIT, B.FIXED_DIST
        self.lc, self.dc = B._FIXED_LIT_CODES, B._FIXED_DIST_CODES
        self.round_base = 8 * ((self.w.bit_length() >> 3) & ~3)
        self.since_match = 0

    def eob(self):
        self.codes.append((self.w.bit_length(), self.lit_v[256], "eob"))
        super().eob()


def steps(s, in_bits, held=False, run0=0):
    """The steps of every lane of the block's first round, each lane decoding once: [(lane, literals of the lane so far % 4, kind of
    the step's own code, follow-up taken, group completed by: None / 1 (the step's literal) / 2 (the follow-up))]."""
    out = []
    lanes = {}
    for c in s.codes:
        k = 0 if c[0] < s.boundary(1) else (c[0] - s.round_base) // (8 * CHUNK)
        if c[2] == "dist":
            k = lanes["last"]
        lanes.setdefault(k, []).append(c)
        lanes["last"] = k
    del lanes["last"]
    for k in sorted(lanes):
        cs, i, nl = [c for c in lanes[k] if c[0] < in_bits or c[2] == "dist"], 0, 0   # (no step starts beyond the input)
        end = min(s.boundary(k + 1), in_bits)
        while i < len(cs):
            at, n, kind = cs[i]
            i += 1
            lit1 = kind in ("lit", "long")
            take = False
            if kind not in ("len", "eob", "bad") and i < len(cs):
                fat, fn, fkind = cs[i]
                take = fkind == "lit" and fat < end and (not held or ((at - s.round_base) & 31) + n <= HELD_MAX)
            done = 1 if lit1 and (nl + 1) % 4 == 0 else 2 if take and (nl + lit1 + 1) % 4 == 0 else None
            out.append((k, nl % 4, kind, take, done))
            nl += lit1 + take
            i += take
            if kind in ("eob", "bad"):
                break
    return out


def _case(out, name, s, cut=None, cap=None):
    out.append((name, s.data(cut), cap, s, 8 * (cut if cut is not None else len(s.data()))))


@functools.lru_cache(maxsize=None)
def directed():
    """(name, stream, cap or None, the Logged builder, bits of input)"""
    out = []
    A, Bb, X = 97, 98, 120

    # every count of literals % 4 at the start of a step x what the step's own code is, a literal behind it; none behind a length.
    # r literals bring the count to r, two to a step; a pair in front of an odd number of them takes the first as its follow-up.
    for r in range(4):
        for kind, front in (("literal", [A]), ("pair", [PC.PAIR]), ("distance", [NOPAIR]), ("length", None)):
            s = Logged()
            s.header()
            s.put(*([PC.MATCH] * (r % 2) + [A] * r))
            if kind == "length":
                s.put(NOPAIR, A, Bb)                # (the code behind a length is its distance; the literal comes behind that)
            else:
                s.put(*front, Bb, PC.MATCH, *front, X, A, PC.MATCH)
            s.eob()
            _case(out, "count-%d-literal-behind-a-%s" % (r, kind), s)

    # a group of four completed by the step's literal (the follow-up opens the next), and by the follow-up
    for lits, name in (([A, Bb, X, A, Bb, X, A, Bb], "both-ways-in-turn"), ([A] * 9, "nine"), ([PC.MATCH, A, Bb, X, A], "first-literal-completes-alone"), ([PC.MATCH, A, Bb, X, A, Bb, A, X, Bb, A, X], "first-literal-completes")):
        s = Logged()
        s.header()
        s.put(*lits, PC.MATCH)
        s.eob()
        _case(out, "group-" + name, s)

    # a literal that starts exactly at the end of a sub-chunk (not taken: the neighbour begins there), and one bit in front of it
    for k in (1, 2, 63):
        for delta in (0, -1, 1):
            for front, fname in (([PC.MATCH, X, A], "literal"), ([PC.PAIR], "pair")):   # (a pair is a step of its own, x its follow-up: so is a)
                s = Logged()
                s.header()
                n_front = 10 if fname == "literal" else 8
                s.pad_to(s.boundary(k) + delta - n_front)
                s.put(*front, Bb, A, X, PC.MATCH, A)
                s.eob()
                _case(out, "literal-at-boundary-%d%+d-behind-a-%s" % (k, delta, fname), s)

    # candidates that are no plain literal of the direct table: the end of the block, a length, a pair, a link, a code of exactly
    # the index bits (taken), no symbol at all
    for name, cand in (("end-of-block", None), ("length", NOPAIR), ("pair", PC.PAIR)):
        s = Logged()
        s.header()
        s.put(A, A, Bb)
        if cand:
            s.put(cand, A, PC.MATCH, cand)
        s.eob()
        _case(out, "candidate-" + name, s)
    for name, cand in (("link-11-bits", 65), ("link-12-bits", 67), ("code-of-10-bits", 126), ("code-of-9-bits", 125)):
        s = Logged(lit=DEEP_V)
        s.header()
        s.put(A, cand, A, Bb, PC.MATCH, cand, cand, X, A)
        s.eob()
        _case(out, "candidate-" + name, s)
    for sym, at in ((286, 1), (287, 3)):
        s = Logged()
        s.fixed_header()
        s.put(*([A, 200, Bb] * 3)[:at], ("code", "lit", sym), A, Bb)
        s.eob()
        _case(out, "candidate-symbol-%d" % sym, s)

    # a literal that ends beyond the input, in the last sub-chunk of a stream: as a step of its own and as a follow-up
    for shift in (0, 1):
        s = Logged(lit=DEEP_V)
        s.header()
        t = (s.w.bit_length() + 900) & ~7
        s.pad_to(t - 8 - 3 * shift - 7)                # (the code of 126 ends in two zeros, as the fill behind the input does)
        s.put(PC.MATCH, X, *([A] * shift), 126, A, A)   # (a pair is a step of its own, x its follow-up)
        s.eob()
        _case(out, "literal-ends-beyond-the-input-%d" % shift, s, cut=t // 8)

    # form (b): the largest pair in front of a literal at every bit offset of a dword
    for off in range(32):
        s = Logged(prefix=33000)
        s.header()
        at = s.round_base + 32 * 12 + off
        s.pad_to(at)
        s.put(BIGPAIR, A)
        s.eob()
        _case(out, "largest-pair-at-bit-%d-of-its-dword" % off, s)

    # more literals in a sub-chunk than a record carries: the round falls back
    s = Logged()
    s.header()
    s.put(*([X] * 200), PC.MATCH, *([A, X] * 70), PC.PAIR, Bb)
    s.eob()
    _case(out, "more-than-127-literals", s)

    # literals no record covers yet, from the block in front
    s = Logged()
    s.header(final=False)
    s.put(*([A] * 7))
    s.eob()
    s.codes = []
    s.header()
    s.put(A, Bb, X, PC.PAIR, A, A)
    s.eob()
    _case(out, "pending-literals-from-the-block-in-front", s)

    # distances checked against the output (the first 32 KiB), literals on both sides of the match: exactly the output, one beyond
    for over in (0, 1):
        s = Logged(prefix=0)
        s.header()
        s.put(A, Bb, X, A, Bb, ("sym", 258, 0) + B._DIST_SYM[5 + over], A, Bb, ("sym", 285, 0) + B._DIST_SYM[6], X, A)
        s.eob()
        _case(out, "distance-%s-the-output" % ("one-beyond" if over else "exactly"), s)

    assert len({c[0] for c in out}) == len(out)
    return tuple(out)


def small_streams(rnd, count=16):
    """`count` streams of 2 .. 4 KiB over the two code sets: runs of literals between matches."""
    out = []
    for c in range(count):
        n = rnd.randrange(2048, 4097)
        s = Logged(prefix=200 + c, lit=DEEP_V if c % 2 else None)
        s.header()
        lits = [97, 98, 120, 121, 122, 126, 65] if c % 2 else [97, 98, 120, 121]
        while s.n_out < n - 300:
            s.put(*[rnd.choice(lits) for _ in range(rnd.choice([0, 1, 1, 2, 3, 6, 11, 40]))], rnd.choice([PC.PAIR, PC.MATCH, NOPAIR, ("sym", 264, 0, 1, 0)]))
        s.put(*([97] * (n - s.n_out)))
        s.eob()
        out.append(s.data())
    return out
