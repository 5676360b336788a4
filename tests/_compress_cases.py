"""Inputs BUILT against the parse of each encoder, and listers of what an encoder wrote (TEST INFRASTRUCTURE, plain Python: no
engine code, and the listers share no code with the engine).

  listers   `lz4_sequences` (an LZ4 block as [(literals, offset, match length)]), `deflate_tokens` (a Deflate stream as blocks of
            literal / (length, distance) tokens, with the code lengths of a dynamic block), `bzip2_blocks` (per block of a bzip2 stream
            the stored CRC, origin pointer, used bytes, tables, selectors, the code lengths of every table and the number of symbols);
  cases     named tuples (family, name, data, prefix, expect): `expect(listing, kind)` asserts what must hold on the listing of
            the engine's output for `data`.  Every expectation follows from how the input was built and from the format -- none from
            an encoder's output.  The number of cases per family is asserted at the end of the module.

Two documented properties of the device parse (csrc/deflate_comp.h, csrc/lz4_comp.h) shape the "must be found" cases: the 64 lanes
of a window read the hash table before any of them enters its position, so a source in the same 64-position window as the match
start is not seen; and positions inside a match beyond the current window are not entered.  So a designed match has its source 64
bytes or more back, in a stretch that is emitted as literals, and few enough positions lie between the two that the entry is still
the table's (seeds are fixed: where a designed match was lost to a hash collision in the emulation, the case was re-seeded).

A lit/len code deeper than 15 is built (family "deep"); for the DISTANCE alphabet none is, and that case is left out.  Only distances
of 64 and more can be designed (the first property), which leaves the 18 distance symbols 12 .. 29; an unlimited depth of 16 needs
17 of them with counts in Fibonacci proportion at least -- 4,180 matches, about 100 KiB as groups of sources and copies -- and
that proportion has a slack of ONE match per level (F(i+2) = F(1) + .. + F(i) + 1), while a designed match is lost whenever one of
the 65 to several thousand positions between source and copy takes its slot in the table of 4,096.  Counts with a margin for
that (a ratio of 1.7 instead of 1.618) come to about 10,000 matches, which does not fit 128 KiB."""
import collections
import heapq
import random
import zlib

import numpy as np

Case = collections.namedtuple("Case", "family name data prefix expect")

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_BITS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_BITS = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DD = [5] * 30


def rand(n, seed, lo=0, hi=256):
    """n seeded random bytes with lo <= value < hi."""
    rnd = random.Random(seed)
    return bytes(rnd.randrange(lo, hi) for _ in range(n))


# ================================================================================================================ lister: LZ4
def lz4_sequences(block, strict=False):
    """[(literals, offset, match length)] of an LZ4 block; the last sequence has offset 0 and match length 0.  strict: the end
    rules of the format asserted -- a block with a match ends in five literals or more, and its last match starts twelve bytes or
    more before the end of the plain text."""
    z, i, out, plain, last_start = bytes(block), 0, [], 0, None
    assert z, "an LZ4 block has one token at least"
    while True:
        tok = z[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = z[i]
                i += 1
                lit += b
                if b != 255:
                    break
        assert i + lit <= len(z), "literals run past the block"
        lits = z[i:i + lit]
        i += lit
        plain += lit
        if i == len(z):
            assert tok & 15 == 0, "the last token names a match"
            out.append((lits, 0, 0))
            break
        offset = z[i] | (z[i + 1] << 8)
        i += 2
        ml = (tok & 15) + 4
        if tok & 15 == 15:
            while True:
                b = z[i]
                i += 1
                ml += b
                if b != 255:
                    break
        out.append((lits, offset, ml))
        last_start = plain
        plain += ml
    if strict and last_start is not None:
        assert len(out[-1][0]) >= 5, "fewer than five literals at the end: %d" % len(out[-1][0])
        assert last_start + 12 <= plain, "the last match starts %d bytes before the end" % (plain - last_start)
    return out


def lz4_expand(seqs, prefix=b""):
    """What the sequences decode to behind `prefix`; every offset is checked against what lies in front of it."""
    out = bytearray(prefix)
    for lits, offset, ml in seqs:
        out += lits
        if ml:
            assert 1 <= offset <= 65535 and offset <= len(out), "offset %d at position %d (prefix %d)" % (offset, len(out) - len(prefix), len(prefix))
            start = len(out) - offset
            if offset >= ml:
                out += out[start:start + ml]
            else:
                out += (bytes(out[start:]) * (ml // offset + 1))[:ml]
    return bytes(out[len(prefix):])


def lz4_matches(seqs):
    """[(position in the block, offset, length, literals in front)] of the matches."""
    pos, out = 0, []
    for lits, offset, ml in seqs:
        pos += len(lits)
        if ml:
            out.append((pos, offset, ml, len(lits)))
        pos += ml
    return out


# ============================================================================================================ lister: Deflate
def _code_table(lengths):
    """{bit string as it lies in the stream: symbol} of the canonical code (RFC 1951 3.2.2)."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    tab = {}
    for s, n in enumerate(lengths):
        if n:
            tab[format(nxt[n], "0%db" % n)] = s
            nxt[n] += 1
    return tab, sorted(set(n for n in lengths if n))


def deflate_tokens(stream):
    """The blocks of a Deflate stream up to the final one: [{"final", "btype", "tokens", "ll", "dd", "bits"}].  A token is a
    literal (int) or (length, distance); a stored block lists its bytes as literals; ll / dd are the code lengths of a dynamic
    block as its header gives them (HLIT / HDIST entries), None otherwise; bits = (first bit, bit behind the block).  The bytes the
    stream occupies: (last block's end + 7) // 8."""
    z = bytes(stream)
    s = "".join(format(b, "08b")[::-1] for b in z)       # s[k] = bit k of the stream, in the order the decoder reads them
    pos, blocks = 0, []

    def bits(n):
        nonlocal pos
        assert pos + n <= len(s), "the stream ends inside a block"
        v = int(s[pos:pos + n][::-1], 2) if n else 0
        pos += n
        return v

    def sym(tab, lens):
        nonlocal pos
        for n in lens:
            k = tab.get(s[pos:pos + n])
            if k is not None and pos + n <= len(s):
                pos += n
                return k
        raise AssertionError("no code at bit %d" % pos)

    while True:
        first = pos
        final, btype = bits(1), bits(2)
        assert btype != 3, "block type 3"
        ll = dd = None
        tokens = []
        if btype == 0:
            pos = (pos + 7) // 8 * 8
            n, nn = bits(16), bits(16)
            assert n ^ nn == 0xFFFF, "LEN / NLEN"
            assert pos // 8 + n <= len(z), "a stored block runs past the stream"
            tokens = list(z[pos // 8:pos // 8 + n])
            pos += 8 * n
        else:
            if btype == 1:
                lt, dt = _code_table(FIXED_LL), _code_table(FIXED_DD)
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits(3)
                ct = _code_table(cl)
                both = []
                while len(both) < hlit + hdist:
                    c = sym(*ct)
                    if c < 16:
                        both.append(c)
                    elif c == 16:
                        assert both, "16 first"
                        both += [both[-1]] * (3 + bits(2))
                    elif c == 17:
                        both += [0] * (3 + bits(3))
                    else:
                        both += [0] * (11 + bits(7))
                assert len(both) == hlit + hdist, "a run past the tables"
                ll, dd = both[:hlit], both[hlit:]
                lt, dt = _code_table(ll), _code_table(dd)
            while True:
                c = sym(*lt)
                if c < 256:
                    tokens.append(c)
                elif c == 256:
                    break
                else:
                    assert c <= 285, "length symbol %d" % c
                    length = LEN_BASE[c - 257] + bits(LEN_BITS[c - 257])
                    d = sym(*dt)
                    assert d <= 29, "distance symbol %d" % d
                    tokens.append((length, DIST_BASE[d] + bits(DIST_BITS[d])))
        blocks.append({"final": final, "btype": btype, "tokens": tokens, "ll": ll, "dd": dd, "bits": (first, pos)})
        if final:
            return blocks


def deflate_expand(blocks):
    out = bytearray()
    for b in blocks:
        for t in b["tokens"]:
            if isinstance(t, int):
                out.append(t)
            else:
                length, distance = t
                start = len(out) - distance
                assert start >= 0, "a match that reaches in front of the output"
                if distance >= length:
                    out += out[start:start + length]
                else:
                    out += (bytes(out[start:]) * (length // distance + 1))[:length]
    return bytes(out)


def deflate_matches(blocks):
    """[(position, length, distance)] of all matches of the stream."""
    pos, out = 0, []
    for b in blocks:
        for t in b["tokens"]:
            if isinstance(t, int):
                pos += 1
            else:
                out.append((pos, t[0], t[1]))
                pos += t[0]
    return out


def huffman_depth(counts):
    """The depth of an unlimited Huffman code over the non-zero counts (ties: the shallower subtree first, as the lower bound)."""
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def litlen_counts(blocks):
    """Counts of the lit/len symbols 0..285 and of the distance symbols 0..29 of a listing (the end-of-block codes included)."""
    ll, dd = [0] * 286, [0] * 30
    for b in blocks:
        for t in b["tokens"]:
            if isinstance(t, int):
                ll[t] += 1
            else:
                ll[257 + max(k for k in range(29) if LEN_BASE[k] <= t[0])] += 1
                dd[max(k for k in range(30) if DIST_BASE[k] <= t[1])] += 1
        ll[256] += 1
    return ll, dd


# ============================================================================================================== lister: BZip2
BLOCK_MAGIC = 0x314159265359
END_MAGIC = 0x177245385090


def bzip2_blocks(stream):
    """(level, [block], combined CRC as stored, bytes consumed).  A block: {"crc", "orig", "n_used", "n_tables", "n_sel", "lengths" --
    one list per table --, "n_sym" -- symbols coded, the end-of-block symbol included --, "bit" -- where its magic starts}.  A parser
    of its own: header fields, selectors, delta-coded lengths, then the symbols group by group until the end-of-block symbol."""
    z = bytes(stream)
    assert z[:3] == b"BZh" and 0x31 <= z[3] <= 0x39
    s = bin(int.from_bytes(b"\x01" + z, "big"))[3:] + "0" * 32
    nbits = len(z) * 8
    pos, blocks = 32, []

    def get(n):
        nonlocal pos
        assert pos + n <= nbits, "the stream ends inside a block"
        v = int(s[pos:pos + n], 2)
        pos += n
        return v

    while True:
        bit = pos
        magic, crc = get(48), get(32)
        if magic == END_MAGIC:
            return z[3] - 0x30, blocks, crc, (pos + 7) // 8
        assert magic == BLOCK_MAGIC, "no block magic at bit %d" % bit
        assert get(1) == 0, "randomised"
        orig, gmap = get(24), get(16)
        n_used = 0
        for g in range(16):
            if gmap & (0x8000 >> g):
                n_used += bin(get(16)).count("1")
        alpha = n_used + 2
        n_tables, n_sel = get(3), get(15)
        assert 2 <= n_tables <= 6 and n_sel >= 1
        mtf, sel = list(range(n_tables)), []
        for _ in range(n_sel):
            c = 0
            while get(1):
                c += 1
            assert c < n_tables, "selector"
            mtf.insert(0, mtf.pop(c))
            sel.append(mtf[0])
        lengths, decode = [], []
        for _ in range(n_tables):
            ln, ls = get(5), []
            for _ in range(alpha):
                while get(1):
                    ln += 1 - 2 * get(1)
                assert 1 <= ln <= 20, "code length %d" % ln
                ls.append(ln)
            lengths.append(ls)
            # canonical codes in (length, symbol) order; a flat look-up over the longest length
            mx, code, last = max(ls), 0, 0
            sym_of, len_of = np.full(1 << mx, -1, np.int32), np.zeros(1 << mx, np.int32)
            for ln2, sy in sorted((l, k) for k, l in enumerate(ls)):
                code <<= ln2 - last
                last = ln2
                assert code < (1 << ln2), "the code lengths are over-subscribed"
                lo = code << (mx - ln2)
                sym_of[lo:lo + (1 << (mx - ln2))] = sy
                len_of[lo:lo + (1 << (mx - ln2))] = ln2
                code += 1
            decode.append((mx, sym_of.tolist(), len_of.tolist()))
        n_sym, done = 0, False
        for g in range(n_sel):
            mx, sym_of, len_of = decode[sel[g]]
            for _ in range(50):
                v = int(s[pos:pos + mx], 2)
                sy = sym_of[v]
                assert sy >= 0, "no code at bit %d" % pos
                pos += len_of[v]
                n_sym += 1
                if sy == alpha - 1:
                    done = True
                    break
            if done:
                assert g == n_sel - 1, "selectors behind the end-of-block symbol"
                break
        assert done and pos <= nbits, "no end-of-block symbol within the selectors"
        blocks.append({"crc": crc, "orig": orig, "n_used": n_used, "n_tables": n_tables, "n_sel": n_sel, "lengths": lengths, "n_sym": n_sym,
                       "bit": bit})


_REV8 = bytes(int("{:08b}".format(i)[::-1], 2) for i in range(256))


def bz_crc(data):
    """CheckSums.bzip2crc32, the MSB-first CRC-32: zlib's with every byte and the result bit-reversed."""
    return int("{:032b}".format(zlib.crc32(bytes(data).translate(_REV8)))[::-1], 2)


def bz_tables_for(n_sym):
    """bzip2's threshold rule, which the engine's host side follows (tables_for, csrc/bzip2_comp.h)."""
    return 2 if n_sym < 200 else 3 if n_sym < 600 else 4 if n_sym < 1200 else 5 if n_sym < 2400 else 6


# ============================================================================================================= Deflate: cases
def _d_universal(x, blocks):
    """What holds for every stream of the Deflate encoders: one block, lengths 3..258, distances 1..32,768 that stay inside the
    text, no match that starts in the last two bytes, and the tokens expand to the input."""
    assert len(blocks) == 1 and blocks[0]["final"] == 1
    for pos, length, dist in deflate_matches(blocks):
        assert 3 <= length <= 258, (pos, length)
        assert 1 <= dist <= 32768 and dist <= pos, (pos, dist)
        assert pos + 3 <= len(x), "a match starts at %d of %d" % (pos, len(x))
        assert pos + length <= len(x)
    assert deflate_expand(blocks) == x


def _find(blocks, lo, hi):
    """The matches that start in [lo, hi)."""
    return [m for m in deflate_matches(blocks) if lo <= m[0] < hi]


# name of a case -> what is added to its seeds: where the emulation lost a designed match to a hash collision (see above)
RESEED = {"repeat-516": 1, "repeat-517": 1, "run-61-between-matches": 1, "run-129-between-matches": 1, "lit9-455-then-a-match-of-40": 2}


def _deflate_cases(reseed=None):
    cases = []
    reseed = RESEED if reseed is None else reseed

    def add(family, name, x, expect):
        def run(blocks, kind, x=x, expect=expect):
            _d_universal(x, blocks)
            if expect is not None:
                expect(blocks, kind)
        cases.append(Case(family, name, x, b"", run))

    # ---- distance limit: A, filler, A again `gap` bytes behind the first
    def gap_case(gap, filler, seed):
        a = rand(40, seed, 1)
        fill = bytes(gap - 40) if filler == "zeros" else rand(gap - 40, seed + 1000, 1)
        x = a + fill + a + rand(3, seed + 2000, 1)

        def expect(blocks, kind):
            hit = _find(blocks, gap, gap + 40)
            if gap <= 32768 and filler == "zeros":
                assert any(d == gap and n >= 38 for _, n, d in hit), ("the designed match is missing", hit)
            if gap > 32768:
                assert not hit, ("a match in the second copy, whose source is out of reach", hit)
        add("distance", "gap-%d-%s" % (gap, filler), x, expect)

    for k, gap in enumerate((32767, 32768, 32769, 65535, 65536, 65537)):
        gap_case(gap, "zeros", 100 + k)
    gap_case(32768, "random", 110)
    gap_case(65536, "random", 111)

    # ---- source at position 0: the distance equals the position
    for k, gap in enumerate((64, 127, 1000)):
        a = rand(40, 120 + k, 1)
        x = a + bytes(gap - 40) + a + rand(3, 130 + k, 1)
        add("position0", "source-at-0-gap-%d" % gap, x,
            lambda blocks, kind, gap=gap: any(p == d == gap and n >= 38 for p, n, d in _find(blocks, gap, gap + 3)) or _fail("no match at distance = position = %d" % gap))

    # ---- length limit: a source of n bytes again 100 bytes later
    for n, seed in ((257, 140), (258, 141), (259, 142), (516, 143), (517, 144), (600, 145)):
        seed += 10000 * reseed.get("repeat-%d" % n, 0)
        src, mid = rand(n, seed), rand(100, seed + 50)
        x = src + mid + src

        def expect(blocks, kind, n=n, x=x):
            want, left = [], n
            while left >= 3:
                want.append((min(left, 258), n + 100))
                left -= want[-1][0]
            got = [(ln, d) for p, ln, d in _find(blocks, n + 100, 2 * n + 100)]
            assert got == want, (got, want)
            assert blocks[0]["tokens"][-(len(want) + left):] == want + list(x[len(x) - left:]), "the copy is not the end of the listing"
        add("length", "repeat-%d" % n, x, expect)

    # ---- matches near the end: the copy ends on the last byte, one and two bytes in front of it; tiny inputs
    for tail in (0, 1, 2):
        a = rand(40, 150 + tail, 1)
        x = a + rand(100, 160 + tail, 1) + a + rand(tail, 170 + tail, 1)
        add("end", "copy-ends-%d-before-the-end" % tail, x,
            lambda blocks, kind, tail=tail: any(d == 140 and n >= 38 and p + n == 180 for p, n, d in _find(blocks, 140, 143)) or _fail("no match that ends at 180"))
    for x in (b"abc", b"abcd", b"abcde", b"aaa", b"aaaa", b"aaaaa", b"abab", b"ababa"):
        add("end", "tiny-%s" % x.decode(), x, None)

    # ---- emitter steps: literal runs of r bytes between two matches, and in front of the end-of-block code with no match
    for k, r in enumerate((61, 62, 63, 64, 65, 126, 127, 128, 129)):
        k += 10000 * reseed.get("run-%d-between-matches" % r, 0)
        s1, s2 = rand(40, 200 + k, 1), rand(40, 220 + k, 1)
        x = s1 + s2 + rand(64, 240 + k, 1) + s1 + rand(r, 260 + k, 1) + s2 + rand(2, 280 + k, 1)

        def expect(blocks, kind, r=r):
            m = [t for t in deflate_matches(blocks) if t[0] >= 144]
            assert [(p, n) for p, n, d in m] == [(144, 40), (184 + r, 40)], m
        add("emitter", "run-%d-between-matches" % r, x, expect)
        y = rand(r, 300 + k, 0, 144)                 # (literals of eight bits: the static block is smaller than the stored one)

        def expect(blocks, kind, r=r):
            assert len(blocks[0]["tokens"]) == r and not deflate_matches(blocks), "a match in random bytes"
            assert kind != "static" or blocks[0]["btype"] == 1
        add("emitter", "run-%d-alone" % r, y, expect)

    # ---- stage flush (static: a literal of the class costs 8 or 9 bits; the stage holds 256 dwords and leaves at 128, that is
    # at 4,096 bits, looked at after every step of up to 64 codes).  All-literal inputs of 8-bit codes around 512 and 1,024 bytes;
    # and m literals of one class -- the first of them a source S -- in front of a copy of S, then a run of one value, which makes
    # the static block smaller than the stored one.  The step that ends the literals carries 3 + c m + (bits of the match) bits
    # and crosses the flush point: of the eight-bit class m = 509 leaves 0 bits in the carried dword with an S of 20 bytes and 1
    # with one of 40 (21 and 22 bits of match; 31 cannot be had: 3 + 8 m + 20 stays below 4,096 up to m = 509 and the next step
    # ends at m = 512), of the nine-bit class m = 463 / 456 / 470 leave 0 / 1 / 31.
    for n in (510, 511, 512, 513, 514, 1022, 1023, 1024, 1025, 1026):
        y = rand(n, 400 + n, 1, 144)

        def expect(blocks, kind, n=n):
            assert len(blocks[0]["tokens"]) == n and not deflate_matches(blocks), "not all literals"
            assert kind != "static" or blocks[0]["btype"] == 1
        add("flush", "lit8-%d" % n, y, expect)

    def match_bits(length, dist):
        ls = max(k for k in range(29) if LEN_BASE[k] <= length)
        ds = max(k for k in range(30) if DIST_BASE[k] <= dist)
        return FIXED_LL[257 + ls] + LEN_BITS[ls] + 5 + DIST_BITS[ds]
    assert 3 + 8 * 509 + match_bits(20, 509) == 4096 and 3 + 8 * 509 + match_bits(40, 509) == 4097
    assert [(3 + 9 * m + match_bits(40, m)) % 32 for m in (463, 456, 470)] == [0, 1, 31]
    for cls, lo, hi, run, slen, ms in ((8, 1, 144, 0, 20, (509,)), (8, 1, 144, 0, 40, (509,)),
                                       (9, 144, 255, 255, 40, (453, 454, 455, 456, 457, 463, 470, 908, 909, 910, 911, 912))):
        for m in ms:
            name = "lit%d-%d-then-a-match-of-%d" % (cls, m, slen)
            seed = 500 + m + 10000 * reseed.get(name, 0)
            src = rand(slen, seed, lo, hi)
            y = src + rand(m - slen, seed + 1000, lo, hi) + src + bytes([run]) * 3000

            def expect(blocks, kind, m=m, y=y, slen=slen):
                t = blocks[0]["tokens"]
                assert t[:m + 1] == list(y[:m]) + [(slen, m)], t[m - 2:m + 3]
                assert kind != "static" or blocks[0]["btype"] == 1
            add("flush", name, y, expect)

    # ---- the stored rule (Deflate+Compress.swift:30-45: stored when 5 + n is not larger than the Huffman block and fits 16 bits)
    for n in (65529, 65530, 65531):
        y = rand(n, 600 + n % 10)
        add("stored", "random-%d" % n, y, lambda blocks, kind, n=n: (blocks[0]["btype"] == 0) == (n <= 65530) or _fail("block type %d" % blocks[0]["btype"]))
    # no match, 100 literals of eight bits and k of nine: the static block has 10 + 8 x 100 + 9 k bits, that is 4 + n bytes for
    # k = 22 and 5 + n for k = 23; 6 + n for k = 31
    for k9, seed in ((22, 610), (23, 611), (31, 612)):
        y = rand(100, seed, 1, 144) + rand(k9, seed + 10, 144, 256)
        static_size = (3 + 8 * 100 + 9 * k9 + 7 + 7) // 8
        assert static_size - (5 + len(y)) == {22: -1, 23: 0, 31: 1}[k9]

        def expect(blocks, kind, k9=k9):
            assert not deflate_matches(blocks)
            assert (blocks[0]["btype"] == 0) == (k9 >= 23), blocks[0]["btype"]
        add("stored", "static-size-%+d" % (static_size - 5 - len(y)), y, expect)
    return cases


def _fail(msg):
    raise AssertionError(msg)


# ---- dynamic only ---------------------------------------------------------------------------------------------------------------
def de_bruijn(k, n):
    """The de Bruijn sequence B(k, n) over 0 .. k - 1 (Lyndon words), with its first n - 1 symbols again at the end: every n-gram
    of the k symbols exactly once."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq + seq[:n - 1]


def alphabet_of(layout):
    """("run", k) / ("gap", k) items from byte value 0 upwards -> the byte values of the runs."""
    at, out = 0, []
    for what, k in layout:
        if what == "run":
            out += list(range(at, at + k))
        at += k
    assert at <= 255
    return out


def zero_runs(lengths):
    """The lengths of the maximal runs of zeros, in order."""
    out, run = [], 0
    for v in list(lengths) + [1]:
        if v == 0:
            run += 1
        elif run:
            out.append(run)
            run = 0
    return out


HEADER_LAYOUTS = [
    [("run", 1), ("gap", 1), ("run", 1), ("gap", 2), ("run", 1), ("gap", 3), ("run", 1), ("gap", 4), ("run", 1), ("gap", 9), ("run", 1), ("gap", 10),
     ("run", 1), ("gap", 11), ("run", 1), ("gap", 12), ("run", 7)],
    [("run", 8), ("gap", 137), ("run", 7)],
    [("run", 2), ("gap", 138), ("run", 3), ("gap", 5), ("run", 6), ("gap", 6), ("run", 4)],
    [("run", 8), ("gap", 139), ("run", 7)],
    [("run", 7), ("gap", 140), ("run", 8)],
    [("run", 3), ("gap", 149), ("run", 6), ("gap", 5), ("run", 2), ("gap", 7), ("run", 4)],
]


def _header_text(layout, cut=None):
    """Fifteen byte values in the de Bruijn order of their triples (no triple twice: no match, every value equally often) and the
    value 255 twice.  With the end-of-block code that is 15 weights of 225 or so and two small ones: in a Huffman code the two small
    ones pair up, their node joins one of the fifteen, and all fifteen come out at four bits, 255 and 256 at five."""
    alpha = alphabet_of(layout)
    assert len(alpha) == 15
    seq = [alpha[v] for v in de_bruijn(15, 3)]
    if cut is not None:
        seq = seq[:cut]
    x = bytes(seq[:1000] + [255] + seq[1000:2000] + [255] + seq[2000:])
    tri = [x[i:i + 3] for i in range(len(x) - 2)]
    assert len(set(tri)) == len(tri), "a triple twice"
    return x, alpha


def _dynamic_cases():
    cases = []

    def add(family, name, x, expect):
        def run(blocks, kind, x=x, expect=expect):
            _d_universal(x, blocks)
            expect(blocks, kind)
        cases.append(Case(family, name, x, b"", run))

    for k, layout in enumerate(HEADER_LAYOUTS):
        x, alpha = _header_text(layout)
        used = [1 if v in alpha or v >= 255 else 0 for v in range(257)]
        gaps = [n for what, n in layout if what == "gap"]
        assert zero_runs(used)[:len(gaps)] == gaps

        def expect(blocks, kind, alpha=alpha, used=used):
            b = blocks[0]
            assert b["btype"] == 2 and not deflate_matches(blocks)
            ll, dd = b["ll"], b["dd"]
            assert len(ll) == 257, "HLIT %d for a block whose highest lit/len symbol is 256" % len(ll)
            assert [1 if v else 0 for v in ll] == used and zero_runs(ll) == zero_runs(used)
            assert set(ll[v] for v in alpha) == {4} and ll[255] == ll[256] == 5, [ll[v] for v in alpha + [255, 256]]
            assert sorted(v for v in dd if v) == [1, 1], ("no match: two fillers complete the distance code", dd)
        add("header", "zero-runs-%s" % "-".join(str(g) for g in gaps), x, expect)

    # one match of 258: the lit/len table reaches symbol 285 (HLIT = 286)
    x, alpha = _header_text(HEADER_LAYOUTS[1], cut=1500)
    x = x + x[1000:1258]

    def expect(blocks, kind, n=len(x)):
        b = blocks[0]
        assert b["btype"] == 2
        assert [(ln, p + ln) for p, ln, d in deflate_matches(blocks)] == [(258, n)], deflate_matches(blocks)
        assert len(b["ll"]) == 286 and b["ll"][285] != 0
    add("header", "one-match-of-258", x, expect)
    return cases


def deep_input(seed, body, with3):
    """`body` random bytes, then Fibonacci-many matches of the lengths 4 .. 15 (ten length symbols, 258 .. 267; with3: and 89 of
    length 3): every match has a source of its own 80 bytes or so in front of it, in literals, and a byte behind it that ends it."""
    rnd = random.Random(seed)
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55] + ([89] if with3 else [])
    lens = [4, 5, 6, 7, 8, 9, 10, 11, 13, 15] + ([3] if with3 else [])
    plan = [ln for ln, c in zip(lens, fib) for _ in range(c)]
    rnd.shuffle(plan)
    out = bytearray(rnd.randbytes(body))
    for ln in plan:
        src = rnd.randbytes(ln + 1)
        out += src + rnd.randbytes(64) + src[:ln] + bytes([src[ln] ^ 0x55])
    return bytes(out)


def _deep_cases():
    """The precondition of both -- an unlimited Huffman code over the lit/len counts of the parse is deeper than 15 -- is asserted
    by the tests on the listing of the static stream (huffman_depth).  The builder limits a code by halving the weights (as bzip2
    does), which can stop below the limit: the first input comes out at 15 bits exactly, the second at 14."""
    cases = []
    for name, x, exact in (("litlen-deeper-than-15", deep_input(700, 100000, False), True),
                           ("litlen-deeper-than-15-halved-further", deep_input(700, 66000, True), False)):
        def expect(blocks, kind, x=x, exact=exact):
            _d_universal(x, blocks)
            if kind == "dynamic":
                b = blocks[0]
                assert b["btype"] == 2 and max(b["ll"]) <= 15
                assert not exact or max(b["ll"]) == 15, max(b["ll"])
                assert sum(1 << (15 - v) for v in b["ll"] if v) == 1 << 15, "the lit/len code is not complete"
        cases.append(Case("deep", name, x, b"", expect))
    return cases


# ================================================================================================================= LZ4: cases
def _l_universal(x, prefix, seqs):
    assert lz4_expand(seqs, prefix) == x          # (checks 1 <= offset <= 65,535 and offset <= position + prefix)
    for lits, offset, ml in seqs[:-1]:
        assert ml >= 4


def _lz4_cases():
    cases = []

    def add(family, name, x, expect, prefix=b""):
        def run(seqs, kind=None, x=x, prefix=prefix, expect=expect):
            _l_universal(x, prefix, seqs)
            if expect is not None:
                expect(seqs)
        cases.append(Case(family, name, x, prefix, run))

    for k, gap in enumerate((65534, 65535, 65536, 65537, 131071, 131072)):
        a = rand(40, 800 + k, 1)
        x = a + bytes(gap - 40) + a + rand(16, 810 + k, 1)

        def expect(seqs, gap=gap):
            hit = [m for m in lz4_matches(seqs) if gap <= m[0] < gap + 40]
            if gap <= 65535:
                assert any(off == gap and ml >= 38 for _, off, ml, _ in hit), ("the designed match is missing", hit)
            else:
                assert not hit, ("a match in the second copy, whose source is out of reach", hit)
        add("offset", "gap-%d" % gap, x, expect)

    # ---- prefix: A opens the block; in the prefix A lies at its first byte ("first") or 65,535 bytes in front of the block ("reach")
    for k, (plen, where) in enumerate(((65535, "first"), (65536, "first"), (65537, "first"), (70000, "first"), (65536, "reach"), (65537, "reach"),
                                       (70000, "reach"))):
        a = rand(40, 820 + k, 1)
        at = 0 if where == "first" else plen - 65535
        prefix = bytes(at) + a + bytes(plen - at - 40)
        x = a + rand(16, 830 + k, 1)

        def expect(seqs, dist=plen - at):
            m = lz4_matches(seqs)
            if dist <= 65535:
                assert m and m[0][:2] == (0, dist) and m[0][2] >= 38, ("the match into the prefix is missing", m)
            else:
                assert not m, ("the copy in the prefix is out of reach", m)
        add("prefix", "prefix-%d-%s" % (plen, where), x, expect, prefix)
    add("prefix", "no-prefix", rand(40, 840, 1) * 3 + rand(16, 841, 1), None)

    # ---- end rules
    period = rand(36, 850, 1)
    for n in range(72, 91):
        add("end", "period-36-cut-%d" % n, (period * 3)[:n], None)
    for n in (12, 13, 14):
        add("end", "one-value-%d" % n, b"x" * n, None)

    # ---- length codes: a literal run of r, then a match of m (token 15 / extension 0 / extension 255 on either side)
    for k, (r, m) in enumerate(((14, 18), (15, 19), (16, 20), (269, 273), (270, 274), (271, 275))):
        k += 10000 * RESEED.get("run-%d-match-%d" % (r, m), 0)
        s1, s2 = rand(40, 860 + k, 1), rand(m, 870 + k, 1)
        x = s1 + s2 + rand(64, 880 + k, 1) + s1 + rand(r, 890 + k, 1) + s2 + rand(16, 900 + k, 1)

        def expect(seqs, r=r, m=m):
            got = [(lits, off, ml) for _, off, ml, lits in lz4_matches(seqs)]
            assert got == [(104 + m, 104 + m, 40), (r, 104 + m + r, m)], got
            assert len(seqs[-1][0]) == 16
        add("lengths", "run-%d-match-%d" % (r, m), x, expect)
    # (a window of random bytes, a window of zeros whose lanes see no zeros in the table yet, then the match: the first property above)
    x = rand(64, 909, 1) + bytes(64 + 70000) + rand(16, 910, 1)
    add("lengths", "match-70000", x, lambda seqs: [(p, off, ml) for p, off, ml, _ in lz4_matches(seqs)] == [(128, 1, 70000)] or _fail(lz4_matches(seqs)))
    return cases


# =============================================================================================================== BZip2: cases
def fibonacci_word(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def thue_morse(n):
    return bytes(97 + (bin(i).count("1") & 1) for i in range(n))


def text16(n, seed):
    """n bytes over sixteen values, no value four times in a row (RLE1 leaves the text as it is)."""
    rnd = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        v = 65 + rnd.randrange(16)
        if len(out) >= 3 and out[-1] == out[-2] == out[-3] == v:
            continue
        out.append(v)
    return bytes(out)


# (seed, length) of text16 whose symbol count behind MTF / RLE2, the end-of-block symbol included, is the key: found by a search
# over lengths with the Python model (bwt_forward / mtf_encode of tests/_bzip2_build.py), and asserted by the module again
BZ_COUNTS = {199: (2000, 199), 200: (2000, 200), 599: (2000, 599), 600: (2000, 600), 1000: (2000, 1002), 1001: (2000, 1003), 1199: (2000, 1205),
             1200: (2000, 1206), 2399: (2000, 2410), 2400: (2000, 2411)}


def bz_symbol_count(x):
    import _bzip2_build as B
    L, _ = B.bwt_forward(x)
    return len(B.mtf_encode(L, sorted(set(x)))) + 1


def _bzip2_cases():
    cases = []

    def add(family, name, x, level=1, n_sym=None):
        def run(listing, kind=None, x=x, level=level, n_sym=n_sym):
            lv, blocks, combined, used = listing
            raw = level * 80000
            parts = [x[i:i + raw] for i in range(0, len(x), raw)]
            assert lv == level and len(blocks) == len(parts)
            for b in blocks:
                assert b["n_sel"] == -(-b["n_sym"] // 50), (b["n_sel"], b["n_sym"])
                assert b["n_tables"] == bz_tables_for(b["n_sym"]), (b["n_tables"], b["n_sym"])
                for ls in b["lengths"]:
                    assert len(ls) == b["n_used"] + 2 and all(1 <= v <= 20 for v in ls)
                    assert sum(1 << (20 - v) for v in ls) <= 1 << 20, "not a prefix code"
            if n_sym is not None:
                assert [b["n_sym"] for b in blocks] == [n_sym]
            for b, p in zip(blocks, parts):
                assert b["crc"] == bz_crc(p), "the stored CRC of the block at bit %d is not that of its raw bytes" % b["bit"]
                assert b["n_used"] >= len(set(p))          # (RLE1 adds count bytes)
            total = 0
            for b in blocks:
                total = (((total << 1) | (total >> 31)) & 0xFFFFFFFF) ^ b["crc"]
            assert combined == total, "the combined CRC"
        cases.append(Case(family, name, x, level, run))

    # ---- RLE1 runs across the cut between raw blocks
    for k, r in enumerate((3, 4, 5, 254, 255, 256, 259, 260, 510)):
        before = k % 6
        head = text16(80000 - before, 1000 + k)
        x = head + bytes([head[-1] ^ 1]) * r + text16(1000, 1020 + k)
        add("rle1-cut", "run-%d-starts-%d-before-the-cut" % (r, before), x)
    head = text16(160000 - 2, 1040)
    add("rle1-cut", "level-2-run-259", head + b"z" * 259 + text16(1000, 1041), level=2)

    # ---- sort ties
    xx = rand(30000, 1050)
    ties = [("xx", xx + xx), ("xxq", xx + xx + b"q"), ("fibonacci-79999", fibonacci_word(79999)), ("fibonacci-80000", fibonacci_word(80000)),
            ("thue-morse-65536", thue_morse(65536)), ("thue-morse-80000", thue_morse(80000)), ("period-7-of-70000", b"abcdefg" * 10000),
            ("period-7-of-70003", (b"abcdefg" * 10001)[:70003]), ("ab-then-c", b"ab" * 39999 + b"c"), ("a255b", (b"a" * 255 + b"b") * 300),
            ("zeros-160001", bytes(160001)), ("runs-of-four", b"".join(bytes([v]) * 4 for v in rand(20000, 1051)))]
    for name, x in ties:
        add("ties", name, x)

    # ---- table and group counts
    for n_sym in sorted(BZ_COUNTS):
        seed, n = BZ_COUNTS[n_sym]
        x = text16(n, seed)
        assert bz_symbol_count(x) == n_sym, (n_sym, seed, n)
        add("counts", "symbols-%d" % n_sym, x, n_sym=n_sym)

    # ---- alphabets
    for n in (1, 4, 5, 256):
        add("alphabet", "one-value-%d" % n, b"k" * n)
    add("alphabet", "all-256-once", bytes(range(256)))
    add("alphabet", "0-and-255", rand(1000, 1060, 0, 2).translate(bytes([0, 255]) + bytes(254)))
    return cases


DEFLATE = _deflate_cases()
DYNAMIC = _dynamic_cases() + _deep_cases()
LZ4 = _lz4_cases()
BZIP2 = _bzip2_cases()

# the capacity cases: names of cases of different kinds, run again with out_cap = size, size - 1, ... (the tests know the sizes)
DEFLATE_CAPACITY = ("gap-32768-zeros", "repeat-517", "run-64-alone", "lit9-463-then-a-match-of-40", "random-65531", "static-size-+0")
DEFLATE_CAPS = (0, -1, -3, -4, -5, None)         # relative to the size; None: out_cap = 0
LZ4_CAPACITY = ("gap-65535", "prefix-65536-reach", "run-270-match-274", "one-value-13")
LZ4_CAPS = (0, -1, "one", None)                  # need, need - 1, 1, 0


def by_name(cases, name):
    hit = [c for c in cases if c.name == name]
    assert len(hit) == 1, name
    return hit[0]


def _count(cases):
    return dict(collections.Counter(c.family for c in cases))


assert _count(DEFLATE) == {"distance": 8, "position0": 3, "length": 6, "end": 11, "emitter": 18, "flush": 24, "stored": 6}, _count(DEFLATE)
assert _count(DYNAMIC) == {"header": 7, "deep": 2}, _count(DYNAMIC)
assert _count(LZ4) == {"offset": 6, "prefix": 8, "end": 22, "lengths": 7}, _count(LZ4)
assert _count(BZIP2) == {"rle1-cut": 10, "ties": 12, "counts": 10, "alphabet": 6}, _count(BZIP2)
for _c in DEFLATE + DYNAMIC + LZ4 + BZIP2:
    assert len(_c.data) <= 200 * 1024, _c.name
for _n in DEFLATE_CAPACITY:
    by_name(DEFLATE, _n)
for _n in LZ4_CAPACITY:
    by_name(LZ4, _n)
