"""Deflate streams BUILT code by code (TEST INFRASTRUCTURE; standard library only).

zlib is a narrow encoder: it never writes the last 262 distances of the format, length 258 as symbol 284 + 31, a length and a
distance code of 48 bits together, code sets deep enough to overflow the decoder's LDS subtables, code-length runs that cross
from the literal lengths into the distance lengths, dozens of blocks inside one sub-chunk, or an error behind tens of kilobytes
of valid data.  This module writes all of those: a linear-time bit writer, the three block types over a small token language,
a header encoder with a stated run policy, random complete code sets with a bias towards comb-shaped (deep) ones,
`random_stream` for the soak tests and `directed_cases` / `directed_streams` for the named corners.

Tokens of a Huffman block:
    int                                   a literal byte
    (length, distance)                    the usual symbols (258 as symbol 285)
    ("sym", lsym, lextra, dsym, dextra)   a length / distance pair by explicit symbol and extra value
    ("code", "lit" | "dist", symbol)      the bare Huffman code of a symbol (reserved symbols, damage placed on purpose)
    ("raw", value, nbits)                 raw bits, LSB first
Codes are assigned as Code.huffmanCodes assigns them (_streams._ref_codes), so incomplete and over-subscribed code-length vectors
mean to the builder what they mean to the reference.
"""
import functools
import random

from _streams import CL_ORDER, _ref_codes

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_BITS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_BITS = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]

FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

_LEN_SYM = [None] * 259      # length -> (symbol, extra value)
for _s in range(29):          # upwards, so that 258 ends as symbol 285 and not as 284 + 31
    for _e in range(1 << LEN_BITS[_s]):
        if LEN_BASE[_s] + _e <= 258:
            _LEN_SYM[LEN_BASE[_s] + _e] = (257 + _s, _e)
_DIST_SYM = [None] * 32769   # distance -> (symbol, extra value)
for _s in range(30):
    for _e in range(1 << DIST_BITS[_s]):
        _DIST_SYM[DIST_BASE[_s] + _e] = (_s, _e)


class BitWriter:
    """LSB-first bit writer over a bytearray with a small accumulator: linear in the number of bits written."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 32:
            self.buf += (self.acc & 0xFFFFFFFF).to_bytes(4, "little")
            self.acc >>= 32
            self.n -= 32

    def code(self, code, n):
        """Huffman codes go MSB-first into the LSB-first stream (RFC 1951 3.1.1)."""
        self.bits(_reverse(code, n), n)

    def align(self):
        self.bits(0, -self.n % 8)

    def bytes(self, data):
        assert self.n % 8 == 0
        self.buf += self.acc.to_bytes(self.n // 8, "little")
        self.acc = self.n = 0
        self.buf += data

    def bit_length(self):
        return len(self.buf) * 8 + self.n

    def data(self):
        return bytes(self.buf) + self.acc.to_bytes((self.n + 7) // 8, "little")


def _reverse(code, n):
    return int(format(code, "0%db" % n)[::-1], 2) if n else 0


def _reversed_codes(lengths):
    """symbol -> (code with its bits reversed, length): ready for BitWriter.bits."""
    return {s: (_reverse(c, n), n) for s, (c, n) in _ref_codes(lengths).items()}


_FIXED_LIT_CODES = _reversed_codes(FIXED_LIT)
_FIXED_DIST_CODES = _reversed_codes(FIXED_DIST)


# ------------------------------------------------------------------------------------------- tokens
def normalise(tokens):
    """Tokens in one form: int | ("sym", lsym, lextra, dsym, dextra) | ("code", ...) | ("raw", ...)."""
    out = []
    for t in tokens:
        if isinstance(t, int) or isinstance(t[0], str):
            out.append(t)
        else:
            length, distance = t
            out.append(("sym",) + _LEN_SYM[length] + _DIST_SYM[distance])
    return out


def expand(tokens, plain):
    """Append what the (normalised, undamaged) tokens decode to."""
    for t in tokens:
        if isinstance(t, int):
            plain.append(t)
        elif t[0] == "sym":
            length = LEN_BASE[t[1] - 257] + t[2]
            distance = DIST_BASE[t[3]] + t[4]
            start = len(plain) - distance
            assert start >= 0, "a match that reaches in front of the output"
            if distance >= length:
                plain += plain[start:start + length]
            else:
                plain += (bytes(plain[start:]) * (length // distance + 1))[:length]
        else:
            raise ValueError("only literal and match tokens have a plain text")


def _write_tokens(w, tokens, lit, dist, eob):
    bits = w.bits
    for t in tokens:
        if isinstance(t, int):
            bits(*lit[t])
        elif t[0] == "sym":
            bits(*lit[t[1]])
            bits(t[2], LEN_BITS[t[1] - 257])
            bits(*dist[t[3]])
            bits(t[4], DIST_BITS[t[3]])
        elif t[0] == "code":
            bits(*(lit if t[1] == "lit" else dist)[t[2]])
        else:
            bits(t[1], t[2])
    if eob:
        bits(*lit[256])


# ------------------------------------------------------------------------------------------- blocks
def stored_block(w, data, final, nlen=None):
    """nlen: what to write in place of ~LEN (the reference checks LEN & NLEN == 0 only)."""
    assert len(data) <= 65535
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
    w.bytes(data)


def fixed_block(w, tokens, final, eob=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    _write_tokens(w, normalise(tokens), _FIXED_LIT_CODES, _FIXED_DIST_CODES, eob)


def header_symbols(lengths, policy="greedy", rnd=None):
    """The code-length vector as symbols of the code-length alphabet: [(symbol, extra value, first index, count)].  The vector is
    literal lengths and distance lengths in one piece, so runs are free to cross from the one into the other.
    policy: "none" (every length on its own), "greedy" (longest run every time), "random" (a random legal choice every time)."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v = lengths[i]
        run = 1
        while i + run < n and lengths[i + run] == v:
            run += 1
        if policy == "none":
            out.append((v, 0, i, 1))
            i += 1
            continue
        if v == 0 and run >= 3:
            k = min(run, 138) if policy == "greedy" else rnd.choice([1, rnd.randrange(3, min(run, 138) + 1), min(run, 138)])
            if k >= 11:
                out.append((18, k - 11, i, k))
            elif k >= 3:
                out.append((17, k - 3, i, k))
            else:
                out.append((0, 0, i, 1))
                k = 1
            i += k
            continue
        prev = i > 0 and lengths[i - 1] == v
        if v != 0 and prev and run >= 3:
            k = min(run, 6) if policy == "greedy" else rnd.choice([0, rnd.randrange(3, min(run, 6) + 1), min(run, 6)])
            if k:
                out.append((16, k - 3, i, k))
                i += k
                continue
        out.append((v, 0, i, 1))
        i += 1
    return out


def dynamic_block(w, tokens, final, lit_lengths, dist_lengths, policy="greedy", rnd=None, cl_lengths=None, cl_symbols=None, eob=True):
    """One dynamic-Huffman block.  lit_lengths (257 .. 286 entries) and dist_lengths (1 .. 32 entries) may be incomplete or
    over-subscribed.  cl_symbols: the header's code-length symbols as [(symbol, extra value), ...] in place of the encoder's own
    (nothing checks that they spell the two vectors); cl_lengths: the 19 lengths of the code-length code in place of a random
    complete code of up to 7 bits over the symbols used.  HCLEN is trimmed.  Returns the header's symbols."""
    rnd = rnd or random.Random(len(lit_lengths) * 33 + len(dist_lengths))
    assert 257 <= len(lit_lengths) <= 288 and 1 <= len(dist_lengths) <= 32
    if cl_symbols is None:
        cl_symbols = header_symbols(list(lit_lengths) + list(dist_lengths), policy, rnd)
    if cl_lengths is None:
        used = sorted({s[0] for s in cl_symbols})
        if len(used) < 2:   # one code of one bit would be an incomplete set, which zlib refuses in a header
            used = sorted(set(used) | {0, 18})[:max(2, len(used))]
        got = random_complete_lengths(rnd, used, 7, rnd.random())
        cl_lengths = [got.get(s, 0) for s in range(19)]
    hclen = max([4] + [k + 1 for k, s in enumerate(CL_ORDER) if cl_lengths[s]])
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lengths) - 257, 5)
    w.bits(len(dist_lengths) - 1, 5)
    w.bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(cl_lengths[s], 3)
    clc = _reversed_codes(cl_lengths)
    for s in cl_symbols:
        w.bits(*clc[s[0]])
        if s[0] >= 16:
            w.bits(s[1], (2, 3, 7)[s[0] - 16])
    _write_tokens(w, normalise(tokens), _reversed_codes(lit_lengths), _reversed_codes(dist_lengths), eob)
    return cl_symbols


# ------------------------------------------------------------------------------------------- code sets
def random_complete_lengths(rnd, symbols, maxbits, deep):
    """A random COMPLETE prefix code over `symbols` with no code longer than maxbits: {symbol: length}.  Leaves are split until
    there is one per symbol; with probability `deep` the deepest leaf that may still be split is taken (towards a comb: few short
    codes, many long ones, the shape that fills second-level tables), otherwise a leaf chosen uniformly.  One symbol alone gets a
    code of one bit (the only incomplete result)."""
    symbols = list(symbols)
    n = len(symbols)
    assert 1 <= n <= 1 << maxbits
    if n == 1:
        return {symbols[0]: 1}
    count = [0] * (maxbits + 1)
    count[1] = 2
    for _ in range(n - 2):
        open_depths = [d for d in range(1, maxbits) if count[d]]
        if rnd.random() < deep:
            d = open_depths[-1]
        else:
            d = rnd.choices(open_depths, [count[k] for k in open_depths])[0]
        count[d] -= 1
        count[d + 1] += 2
    lengths = [d for d in range(1, maxbits + 1) for _ in range(count[d])]
    rnd.shuffle(symbols)
    return dict(zip(symbols, lengths))


def is_complete(lengths):
    return sum(1 << (15 - l) for l in lengths if l) == 1 << 15


def comb(symbols_short, symbols_long, long_bits=15):
    """{symbol: length}: codes of 1, 2, 3 ... bits for symbols_short in turn, long_bits for every symbol of symbols_long."""
    d = {s: k + 1 for k, s in enumerate(symbols_short)}
    d.update({s: long_bits for s in symbols_long})
    return d


def vector(lengths, n):
    return [lengths.get(s, 0) for s in range(n)]


# ------------------------------------------------------------------------------------------- random streams
LENGTHS = [3, 3, 4, 5, 10, 11, 12, 13, 18, 19, 20, 34, 35, 36, 66, 67, 68, 130, 131, 132, 162, 163, 226, 227, 228, 257, 258, 258]
DISTANCES = [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 384, 385,
             512, 513, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 3072, 3073, 3328, 3329, 4096, 4097, 6144, 6145, 8192, 8193, 12288,
             12289, 16384, 16385, 24576, 24577, 32506, 32507, 32767, 32768, 32768]


def _random_tokens(rnd, style, have, want):
    """Tokens that add at most `want` bytes to an output of `have` bytes.  style 0: mixed; 1: match-heavy; 2: literal-only."""
    tokens, added = [], 0
    alphabet = rnd.choice([256, 256, 20, 3])
    while added < want:
        if style != 2 and have + added > 0 and want - added >= 3 and rnd.random() < (0.9 if style == 1 else 0.3):
            pick = rnd.randrange(8)
            length = rnd.randrange(3, 259) if pick == 0 else rnd.choice(LENGTHS)
            length = min(length, want - added)
            pick = rnd.randrange(8)
            reach = min(have + added, 32768)
            if pick == 0:
                distance = reach                          # exactly to the start of the output / the whole window
            elif pick == 1:
                distance = rnd.randrange(1, reach + 1)
            else:
                distance = min(rnd.choice(DISTANCES), reach)
            if length == 258 and rnd.randrange(2):
                tokens.append(("sym", 284, 31) + _DIST_SYM[distance])
            else:
                tokens.append((length, distance))
            added += length
        else:
            for _ in range(min(want - added, rnd.choice([1, 1, 2, 5, 40]))):
                tokens.append(rnd.randrange(alphabet))
                added += 1
    return tokens, added


def _used_symbols(tokens):
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(t)
        else:
            lit.add(t[1])
            dist.add(t[3])
    return lit, dist


def random_code_sets(rnd, tokens):
    """Complete code sets (which zlib accepts as well) over the symbols the tokens use and a random number of others: one
    distance symbol alone gets the one-bit code, no distance symbol no code at all."""
    lit_used, dist_used = _used_symbols(tokens)
    others = [s for s in range(286) if s not in lit_used]
    lit_syms = sorted(lit_used) + rnd.sample(others, rnd.choice([0, 0, min(5, len(others)), rnd.randrange(len(others) + 1), len(others)]))
    if len(lit_syms) < 2:
        lit_syms.append(rnd.choice(others))
    others = [s for s in range(30) if s not in dist_used]
    dist_syms = sorted(dist_used) + rnd.sample(others, rnd.choice([0, 0, min(3, len(others)), rnd.randrange(len(others) + 1), len(others)]))
    deep = rnd.choice([0.0, 0.3, 0.9, 0.99])
    lit = random_complete_lengths(rnd, lit_syms, rnd.choice([9, 12, 15, 15]), deep)
    dist = random_complete_lengths(rnd, dist_syms, rnd.choice([6, 15, 15]), deep) if dist_syms else {}
    hlit = rnd.choice([max(lit) + 1, 286]) if max(lit) >= 256 else 257
    hdist = rnd.choice([max(dist) + 1, 30]) if dist else rnd.choice([1, 1, 30])
    return vector(lit, max(hlit, 257)), vector(dist, hdist)


def random_stream(rnd, target, style=None):
    """(stream, plain, body_len): blocks of all three types that decode to `target` bytes; body_len is where the final block ends
    (a few bytes may follow it).  style 0: mixed; 1: match-heavy; 2: literal-only; 3: tiny (blocks of 0 .. 5 tokens and empty stored
    blocks between them)."""
    style = rnd.randrange(4) if style is None else style
    w, plain = BitWriter(), bytearray()
    while True:
        left = target - len(plain)
        if style == 3:
            want = min(left, rnd.randrange(0, 6) * rnd.choice([1, 1, 1, 40]))
        else:
            want = min(left, rnd.choice([0, 1, 50, 700, 3000, 20000, 66000, 200000]))
        final = want == left and (left == 0 or rnd.randrange(4) > 0)
        kind = rnd.randrange(8 if style != 3 else 4)
        if kind == 0 or (style == 3 and kind == 1):
            data = rnd.randbytes(0 if kind == 1 else min(want, 65535))
            stored_block(w, data, final and len(data) == want)
            final = final and len(data) == want
            plain += data
        else:
            tokens, _ = _random_tokens(rnd, 0 if style == 3 else style, len(plain), want)
            tokens = normalise(tokens)
            if kind in (2, 3):
                fixed_block(w, tokens, final)
            else:
                lit, dist = random_code_sets(rnd, tokens)
                dynamic_block(w, tokens, final, lit, dist, rnd.choice(["none", "greedy", "random", "random"]), rnd)
            expand(tokens, plain)
        if final:
            break
    body = w.data()
    assert len(plain) == target
    return body + (rnd.randbytes(rnd.randrange(1, 9)) if rnd.randrange(4) == 0 else b""), bytes(plain), len(body)


# ------------------------------------------------------------------------------------------- directed streams
class Case:
    """name, stream, plain (None where the stream is an error case), body_len, the status the case was built for, and whether its
    code sets are all ones zlib accepts."""

    def __init__(self, name, stream, plain, body_len, status, zlib_ok):
        self.name, self.stream, self.plain, self.body_len, self.status, self.zlib_ok = name, stream, plain, body_len, status, zlib_ok


E_LENGTHS, E_BLOCK_TYPE, E_SYMBOL, E_NOT_FOUND, E_TRAP = 101, 102, 103, 104, 900   # include/swc_status.h


def _text(rnd, n):
    """n bytes that compress a little: words of a small alphabet."""
    words = [bytes(rnd.randrange(97, 123) for _ in range(rnd.randrange(2, 9))) for _ in range(64)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
    return bytes(out[:n])


def _prefix(w, plain, n, rnd):
    """Non-final blocks of every type that add exactly n bytes: literals, matches at every kind of distance."""
    end = len(plain) + n
    while len(plain) < end:
        want = min(end - len(plain), rnd.choice([1, 40, 700, 3000, 9000]))
        kind = rnd.randrange(4)
        if kind == 0:
            data = _text(rnd, want)
            stored_block(w, data, False)
            plain += data
            continue
        tokens, _ = _random_tokens(rnd, rnd.choice([0, 0, 1, 2]), len(plain), want)
        tokens = normalise(tokens)
        if kind == 1:
            fixed_block(w, tokens, False)
        else:
            lit, dist = random_code_sets(rnd, tokens)
            dynamic_block(w, tokens, False, lit, dist, "random", rnd)
        expand(tokens, plain)


def _extreme_pairs():
    """Every length symbol and every distance symbol at extra = 0 and extra = max."""
    lens = [(257 + s, e) for s in range(29) for e in sorted({0, (1 << LEN_BITS[s]) - 1})]
    dists = [(s, e) for s in range(30) for e in sorted({0, (1 << DIST_BITS[s]) - 1})]
    return [("sym",) + lens[k % len(lens)] + dists[k % len(dists)] for k in range(max(len(lens), len(dists)) * 2 - 1)]


DEEP_LIT = comb([256, 101, 32, 257, 116, 285, 97], [s for s in range(256) if s not in (101, 32, 116, 97)] + [258, 270, 284, 283])
DEEP_DIST = comb([0, 3, 29, 10, 28, 1, 20], [s for s in range(30) if s not in (0, 3, 29, 10, 28, 1, 20)])
assert is_complete(DEEP_LIT.values()) and len(DEEP_LIT) == 263 and not is_complete(DEEP_DIST.values())


def _deep_tokens(rnd, plain_len, lit, dist, n):
    """Tokens over exactly the symbols of the two sets: every long code is used."""
    lits = [s for s in lit if s < 256]
    lens = [s for s in lit if s > 256]
    dists = [s for s in dist if DIST_BASE[s] <= plain_len]
    tokens = list(lits)
    for _ in range(n):
        if rnd.randrange(3) and dists:
            ls, ds = rnd.choice(lens), rnd.choice(dists)
            de = min(rnd.choice([0, (1 << DIST_BITS[ds]) - 1, rnd.randrange(1 << DIST_BITS[ds])]), plain_len - DIST_BASE[ds])
            tokens.append(("sym", ls, rnd.choice([0, (1 << LEN_BITS[ls - 257]) - 1]), ds, de))
        else:
            tokens.append(rnd.choice(lits))
    return tokens


def _finish(name, w, plain, status=0, zlib_ok=True, tail=b"", cut=None):
    body = w.data()
    if cut is not None:
        body = body[:cut]
    return Case(name, body + tail, bytes(plain) if status == 0 else None, len(body), status, zlib_ok)


def _error_cases():
    """Six kinds of error, each behind 0 .. 70,000 bytes that decode: the fast path has committed rounds when it meets them."""
    out = []
    for depth in (0, 1, 100, 5000, 40000, 70000):
        for kind, status in (("distance-beyond-output", E_TRAP), ("fixed-literal-286", E_SYMBOL), ("distance-symbol-30", E_SYMBOL),
                             ("stored-len-and-nlen", E_LENGTHS), ("block-type-3", E_BLOCK_TYPE), ("cut-in-distance-extra-bits", E_NOT_FOUND)):
            if kind == "distance-beyond-output" and depth >= 32768:
                continue
            rnd = random.Random("%s %d" % (kind, depth))
            w, plain = BitWriter(), bytearray()
            _prefix(w, plain, depth, rnd)
            lead = [rnd.randrange(97, 123) for _ in range(rnd.randrange(3))] if depth else []
            cut = None
            if kind == "distance-beyond-output":
                d = len(plain) + len(lead) + 1
                if rnd.randrange(2):
                    fixed_block(w, lead + [("sym", 260, 0) + _DIST_SYM[d], 65], True)
                else:
                    tokens = normalise(lead + [("sym", 260, 0) + _DIST_SYM[d], 65])
                    dynamic_block(w, tokens, True, *random_code_sets(rnd, tokens), "random", rnd)
            elif kind == "fixed-literal-286":
                fixed_block(w, lead + [("code", "lit", 286), 65], True)
            elif kind == "distance-symbol-30":
                fixed_block(w, lead + [66, ("code", "lit", 257), ("code", "dist", 30), 65], True)
            elif kind == "stored-len-and-nlen":
                fixed_block(w, lead, False)
                stored_block(w, b"abc", True, nlen=0xFFFD)       # LEN 3: one bit in common
            elif kind == "block-type-3":
                fixed_block(w, lead, False)
                w.bits(1, 1)
                w.bits(3, 2)
                w.bits(0, 13)
            else:
                fixed_block(w, lead + [66] * 4, False)
                w.bits(1, 1)
                w.bits(1, 2)
                w.bits(*_FIXED_LIT_CODES[257])
                w.bits(*_FIXED_DIST_CODES[28])     # thirteen extra bits follow; the stream ends inside the byte the code ends in
                cut = (w.bit_length() + 7) // 8
            out.append(_finish("error-%s-behind-%d" % (kind, depth), w, plain, status, cut=cut))
    return out


@functools.lru_cache(maxsize=None)
def directed_cases():
    """The named corners, one or more per structure of the decoder that zlib's streams do not reach."""
    out = []
    rnd = random.Random(0xD1EC7ED)
    base = _text(rnd, 65535)

    # every length and distance symbol at its lowest and highest extra value
    pairs = _extreme_pairs()
    for form in ("dynamic", "fixed"):
        w, plain = BitWriter(), bytearray()
        stored_block(w, base[:32768], False)
        plain += base[:32768]
        if form == "fixed":
            fixed_block(w, pairs, True)
        else:
            lit = random_complete_lengths(rnd, range(286), 15, 0.5)
            dist = random_complete_lengths(rnd, range(30), 15, 0.5)
            dynamic_block(w, pairs, True, vector(lit, 286), vector(dist, 30), "random", rnd)
        expand(pairs, plain)
        out.append(_finish("every-symbol-at-both-extremes-" + form, w, plain))

    w, plain = BitWriter(), bytearray()
    tokens = [65, 66, 67, ("sym", 284, 31, 0, 0), (258, 1), ("sym", 284, 31, 0, 0), ("sym", 284, 30, 0, 0), 68]
    fixed_block(w, tokens[:3] + [("sym", 284, 31, 2, 0), (258, 3)], False)
    expand(normalise(tokens[:3] + [("sym", 284, 31, 2, 0), (258, 3)]), plain)
    lit = comb([284, 65, 256], [66, 67, 68, 285], 5)
    dynamic_block(w, tokens[:3] + tokens[3:] * 40, True, vector(lit, 286), [1])
    expand(normalise(tokens[:3] + tokens[3:] * 40), plain)
    out.append(_finish("length-258-as-284-plus-31", w, plain))

    # the largest distance, at the first position where it is legal, one behind it, and behind a window that has slid
    for at in (32768, 32769, 65536 + 7):
        w, plain = BitWriter(), bytearray()
        _prefix(w, plain, at, random.Random(at))
        tokens = normalise([(258, 32768), 33, (3, 32768), (4, 32767), ("sym", 284, 31, 29, 8191), 34, (100, 32768)])
        lit, dist = random_code_sets(random.Random(at + 1), tokens)
        dynamic_block(w, tokens, True, lit, dist, "greedy")
        expand(tokens, plain)
        out.append(_finish("distance-32768-at-output-%d" % at, w, plain, tail=b"\x00\xff\x55" if at == 32769 else b""))

    # 15 + 5 + 15 + 13 bits: a run of the longest length / distance pairs over more than two rounds of 4,352 bytes, so that one
    # straddles ends of sub-chunks and of rounds at many bit positions (a one-bit literal now and then shifts the phase)
    w, plain = BitWriter(), bytearray()
    stored_block(w, base[:32768], False)
    plain += base[:32768]
    lit = comb([120, 256] + list(range(98, 109)), [281, 282, 283, 284])
    dist = comb(range(14), [28, 29])
    assert is_complete(lit.values()) and is_complete(dist.values())
    tokens = []
    for k in range(1500):
        ls, ds = 281 + (k % 4 if k % 8 == 0 else 0), 28 + (k // 3) % 2
        tokens.append(("sym", ls, rnd.choice([0, 1, 2, 5]), ds, rnd.choice([0, 8191, rnd.randrange(8192)])))
        if k % 37 == 5:
            tokens.append(120)
    dynamic_block(w, tokens, True, vector(lit, 286), vector(dist, 30))
    expand(tokens, plain)
    assert w.bit_length() - 32773 * 8 > 2 * 4352 * 8
    out.append(_finish("pairs-of-48-bits-over-several-rounds", w, plain))

    # deep code sets: more second-level entries than the LDS subtable holds, on either side and on both
    shallow_lit = random_complete_lengths(rnd, sorted(DEEP_LIT), 9, 0.0)
    shallow_dist = random_complete_lengths(rnd, sorted(DEEP_DIST), 5, 0.0)
    for name, lit, dist in (("deep-literal-set-256-long-codes", DEEP_LIT, shallow_dist), ("deep-distance-set-15-bit-codes", shallow_lit, DEEP_DIST),
                            ("deep-sets-on-both-sides", DEEP_LIT, DEEP_DIST)):
        w, plain = BitWriter(), bytearray()
        stored_block(w, base[:40000], False)
        plain += base[:40000]
        tokens = _deep_tokens(rnd, len(plain), lit, dist, 3000)
        dynamic_block(w, tokens, True, vector(lit, 286), vector(dist, 30), "greedy", rnd)
        expand(tokens, plain)
        out.append(_finish(name, w, plain, zlib_ok=is_complete(dist.values())))

    w, plain = BitWriter(), bytearray()
    tokens = normalise(list(range(256)) + [(3 + k, 1 + 5 * k) for k in range(40)] + [(258, 256), ("sym", 284, 31, 0, 0)])
    dynamic_block(w, tokens, True, [11] * 286, [5] * 30, "greedy", rnd)
    expand(tokens, plain)
    out.append(_finish("286-codes-of-11-bits", w, plain, zlib_ok=False))

    # the same symbols in three consecutive blocks under three different deep sets: subtables of the block before must not leak
    w, plain = BitWriter(), bytearray()
    stored_block(w, base[:33000], False)
    plain += base[:33000]
    syms, dsyms = sorted(DEEP_LIT), sorted(DEEP_DIST)
    tokens = _deep_tokens(rnd, len(plain), DEEP_LIT, DEEP_DIST, 400)
    for k in range(3):
        r2 = random.Random(k)
        lit = dict(zip(r2.sample(syms, len(syms)), sorted(DEEP_LIT.values())))
        dist = random_complete_lengths(r2, dsyms, 15, 0.95)
        dynamic_block(w, tokens, k == 2, vector(lit, 286), vector(dist, 30), ("greedy", "none", "random")[k], r2)
        expand(tokens, plain)
    out.append(_finish("same-symbols-three-blocks-three-deep-sets", w, plain))

    # code-length runs that cross from the literal lengths into the distance lengths
    for sym in (16, 17, 18):
        lit = [0] * 286
        for s in (65, 66, 67, 256, 257, 258, 259, 260):
            lit[s] = 3
        if sym == 16:
            lit = lit[:257 + 28]
            lit[281:285] = [4, 4, 4, 4]      # 281 .. 284 at 4 bits: over-subscribed by nothing used below
            lit[65] = lit[66] = 4
            lit[67] = 0
            dist = [4, 4, 4, 4] + [2, 2, 2]
        else:
            lit = lit[:261] + [0] * (3 if sym == 17 else 20)
            dist = [0] * (4 if sym == 17 else 9) + [1, 1]
        w, plain = BitWriter(), bytearray()
        far = (1, 0) if sym == 16 else (len(dist) - 1, len(dist) - 2)
        tokens = normalise([65, 66] * 20 + [("sym", 257, 0, far[0], 0), ("sym", 258, 0, far[1], 0)])
        head = dynamic_block(w, tokens, True, lit, dist, "greedy")
        assert [h for h in head if h[0] == sym and h[2] < len(lit) < h[2] + h[3]], "no run of symbol %d crosses the boundary" % sym
        expand(tokens, plain)
        out.append(_finish("code-length-run-%d-crosses-into-distances" % sym, w, plain, zlib_ok=is_complete(lit) and is_complete(dist)))

    # HCLEN at both ends.  4: only 16, 17, 18 and 0 can have a code, so every length is zero and the first symbol is not found
    w, plain = BitWriter(), bytearray()
    fixed_block(w, list(b"four"), False)
    plain += b"four"
    dynamic_block(w, [("raw", 0, 16)], True, [0] * 257, [0], "greedy", cl_lengths=[0] * 16 + [0, 1, 1], eob=False)
    out.append(_finish("hclen-4-every-length-zero", w, plain, E_NOT_FOUND))
    w, plain = BitWriter(), bytearray()
    tokens = list(b"hclen five: 256 codes of eight bits")
    dynamic_block(w, tokens, True, [8] * 255 + [0, 8], [0], "greedy", cl_lengths=[2] + [0] * 7 + [2] + [0] * 7 + [2, 3, 3])
    expand(tokens, plain)
    out.append(_finish("hclen-5", w, plain))
    w, plain = BitWriter(), bytearray()
    lit = comb([256, 97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 259, 263], [110, 111])
    tokens = (list(range(97, 108)) + [110, 111]) * 3 + [(5, 2), (9, 1)]
    dynamic_block(w, tokens, True, vector(lit, 264), [1, 1], "none", cl_lengths=[1, 2, 3, 6, 6, 6] + [7] * 10 + [0, 0, 0])
    expand(normalise(tokens), plain)
    out.append(_finish("hclen-19-code-length-codes-of-7-bits", w, plain))

    w, plain = BitWriter(), bytearray()
    lit = [0] * 286
    lit[40], lit[41], lit[256], lit[285] = 2, 2, 2, 2
    tokens = [40, 41, 40, (258, 2), 41]
    head = dynamic_block(w, tokens, True, lit, [1, 1], "greedy")
    assert (18, 127) in [h[:2] for h in head]
    expand(normalise(tokens), plain)
    out.append(_finish("run-of-138-zeros", w, plain))

    w, plain = BitWriter(), bytearray()
    fixed_block(w, list(b"sixteen"), False)
    plain += b"sixteen"
    dynamic_block(w, [("raw", 0, 16)], True, [0] * 257, [0], cl_symbols=[(16, 0), (18, 127), (18, 105), (1, 0), (1, 0)], eob=False)
    out.append(_finish("symbol-16-first", w, plain, E_SYMBOL))

    w, plain = BitWriter(), bytearray()
    tokens = [7, (3, 1), 9, 9, (258, 1), 7, ("sym", 284, 31, 0, 0)] * 300
    lit = random_complete_lengths(rnd, [7, 9, 256, 257, 284, 285], 6, 0.5)
    dynamic_block(w, tokens, True, vector(lit, 286), [1])
    expand(normalise(tokens), plain)
    out.append(_finish("one-distance-code-of-one-bit", w, plain))

    w, plain = BitWriter(), bytearray()
    tokens = list(_text(rnd, 6000))
    lit = random_complete_lengths(rnd, sorted(set(tokens)) + [256], 15, 0.8)
    dynamic_block(w, tokens, True, vector(lit, 257), [0], "random", rnd)
    expand(tokens, plain)
    out.append(_finish("no-distance-code-literals-only", w, plain))

    w, plain = BitWriter(), bytearray()
    _prefix(w, plain, 6000, rnd)
    lit = random_complete_lengths(rnd, [65, 66, 256, 257], 3, 0.0)
    dynamic_block(w, [65, 66, ("code", "lit", 257), ("raw", 0, 9), 66], True, vector(lit, 258), [0])
    out.append(_finish("no-distance-code-and-a-length-symbol", w, plain, E_NOT_FOUND))

    # the round structure: many blocks inside one sub-chunk, stored blocks at every bit alignment and of the largest size
    w, plain = BitWriter(), bytearray()
    for _ in range(200):
        fixed_block(w, [], False)
    tokens, _ = _random_tokens(rnd, 0, 0, 9000)
    fixed_block(w, tokens, False)
    for _ in range(200):
        fixed_block(w, [], False)
    fixed_block(w, [(258, 9000), 1, 2, 3], True)
    expand(normalise(tokens + [(258, 9000), 1, 2, 3]), plain)
    out.append(_finish("200-empty-fixed-blocks-then-data", w, plain))

    w, plain = BitWriter(), bytearray()
    seen = set()
    for fill in (b"", b"store"):
        for nine in range(8):       # a fixed block of 10 + 8 k + (number of nine-bit literals) bits, begun on a byte boundary
            tokens = list(b"align %d " % nine) + [200 + nine] * nine + ([(4, 3)] if plain else [])
            fixed_block(w, tokens, False)
            expand(normalise(tokens), plain)
            seen.add(w.bit_length() % 8)
            stored_block(w, fill, False)
            plain += fill
    assert len(seen) == 8
    stored_block(w, b"", True)
    out.append(_finish("stored-blocks-at-each-bit-alignment", w, plain))

    w, plain = BitWriter(), bytearray()
    fixed_block(w, list(b"head "), False)
    stored_block(w, base, False)
    fixed_block(w, [(258, 32768), (30, 65535 - 32768 + 1)], False)
    stored_block(w, base[::-1], False)
    stored_block(w, b"", False)
    fixed_block(w, [(258, 32768), (258, 1), 0], True)
    plain += b"head " + base
    expand(normalise([(258, 32768), (30, 65535 - 32768 + 1)]), plain)
    plain += base[::-1]
    expand(normalise([(258, 32768), (258, 1), 0]), plain)
    out.append(_finish("stored-blocks-of-65535-bytes", w, plain))

    # the longest header: 286 + 30 lengths, each on its own, the frequent ones under code-length codes of 7 bits
    w, plain = BitWriter(), bytearray()
    lit = random_complete_lengths(rnd, range(286), 15, 0.0)
    dist = random_complete_lengths(rnd, range(30), 15, 0.0)
    freq = sorted(set(lit.values()) | set(dist.values()), key=lambda v: -(list(lit.values()) + list(dist.values())).count(v))
    cl = dict(zip(freq, sorted(random_complete_lengths(rnd, freq, 7, 1.0).values(), reverse=True)))
    tokens = list(b"a short body") + [(12, 12)]
    start = w.bit_length()
    dynamic_block(w, [], False, vector(lit, 286), vector(dist, 30), "none", cl_lengths=vector(cl, 19))
    assert w.bit_length() - start > 3 * 68 * 8 and max(cl.values()) == 7
    dynamic_block(w, tokens, True, vector(lit, 286), vector(dist, 30), "none", cl_lengths=vector(cl, 19))
    expand(normalise(tokens), plain)
    out.append(_finish("longest-header-316-lengths-without-runs", w, plain, tail=b"\xaa"))

    out += _error_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def directed_streams():
    """(name, stream, plain or None)"""
    return [(c.name, c.stream, c.plain) for c in directed_cases()]
