"""The cases of the placement tests (test_gpu_placement.py on the device through _placed.PlacedBatch, test_placement_emulation.py on
the host emulation), group by group, and where each case is placed.  TEST INFRASTRUCTURE ONLY.

Every expectation comes from the oracle (tests/_oracle.py), is computed once at import and never changed; the engine has no say.  No
case is filtered by status: the module asserts at import that the oracle says 0 on every case but the named error cases, whose status
it asserts not to be 0.  Shapes are the smallest at which each path is live (nothing above about 140 KB but the two Adler-32 jobs)."""
import bz2
import collections
import ctypes as C
import random
import zlib

import _bzip2_build as BB
import _deflate_build as DB
import _lzma_build as LB
import _oracle as O
import _soak as K
import _streams as S
from swcompression_amd import corpus

LZ4_STORED = 2
O.lib.refcpu_delta_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p]
O.lib.refcpu_delta_decode.restype = None


class Case:
    """One unit and what a job over it must report.  status / out_len / in_consumed / data: as _placed.PlacedBatch.verify reads them
    (None: not compared).  aux_out: what the job leaves in `aux`, where the codec documents the field as OUT (bzip2: the CRC-32 of the
    block's output).  hot: the full 16 x 16 cross of residues.  at: a residue pair of its own.  error: one of the named error cases --
    the oracle's status is not 0.  lzma: (lc, lp, pb, dictionary size, declared size) of a raw LZMA job.  source: (prefix, block) an
    encoder's unit was made of."""

    def __init__(self, name, unit, cap, status, data, out_len=None, in_consumed=None, aux=0, extra=0, dict_value=0, dictionary=None,
                 prefix=None, hot=False, at=None, error=False, codec=None, in_place=False, lzma=None, source=None, aux_out=None):
        self.name, self.unit, self.cap, self.status, self.data = name, bytes(unit), int(cap), status, data
        self.out_len, self.in_consumed, self.aux, self.extra, self.dict_value = out_len, in_consumed, aux, extra, dict_value
        self.dictionary, self.prefix, self.hot, self.at, self.error, self.codec = dictionary, prefix, hot, at, error, codec
        self.in_place, self.lzma, self.source, self.aux_out = in_place, lzma, source, aux_out


def _ok(name, unit, oracle, cap=None, **kw):
    """A case the oracle decodes: status 0, its bytes, its consumed input."""
    st, out = oracle[0], oracle[1]
    assert st == 0, "%s: the oracle says %d" % (name, st)
    return Case(name, unit, max(len(out), 1) if cap is None else cap, 0, out, len(out), oracle[2] if len(oracle) > 2 else len(unit), **kw)


def _short(name, unit, oracle, cap, **kw):
    """A valid unit in a capacity too small: SWC_E_CAPACITY, out_len = the bytes required (include/swc_hip.h), the first `cap` bytes."""
    st, out = oracle[0], oracle[1]
    assert st == 0 and cap < len(out), name
    return Case(name, unit, cap, 901, out, len(out), None, **kw)


def _error(name, unit, oracle, cap, **kw):
    assert oracle[0] not in (0, 901), "%s: the oracle says %d" % (name, oracle[0])
    return Case(name, unit, cap, oracle[0], None, error=True, **kw)


# ------------------------------------------------------------------------------------------------------------------------- Deflate
def _deflate():
    out = []
    for n in (0, 1, 15, 16, 17, 2047, 2048, 2049, 6145):
        z = corpus.deflate_raw(corpus.p_text(n, 700 + n))
        out.append(_ok("text-%d" % n, z, O.deflate(z)))
    z = corpus.deflate_raw(corpus.p_text(5000, 31))
    out.append(_ok("text-5000", z, O.deflate(z), hot=True))
    z70 = corpus.deflate_raw(corpus.p_mix(70001, 32))
    out.append(_ok("mix-70001", z70, O.deflate(z70), hot=True))
    zs = corpus.deflate_raw(corpus.p_rand(7001, 33), 0)
    assert zs[0] & 6 == 0
    out.append(_ok("stored-7001", zs, O.deflate(zs), hot=True))
    # one dynamic block with 15-bit distance codes behind a stored block (tests/_deflate_build.py)
    rnd = random.Random(0x9A)
    w, plain = DB.BitWriter(), bytearray(corpus.p_text(2000, 34))
    DB.stored_block(w, bytes(plain), False)
    lit = DB.random_complete_lengths(rnd, sorted(DB.DEEP_LIT), 9, 0.0)
    tokens = DB._deep_tokens(rnd, len(plain), lit, DB.DEEP_DIST, 400)
    DB.dynamic_block(w, tokens, True, DB.vector(lit, 286), DB.vector(DB.DEEP_DIST, 30), "greedy", rnd)
    DB.expand(tokens, plain)
    assert max(DB.DEEP_DIST.values()) == 15
    built = w.data()
    exp = O.deflate(built)
    assert exp[:2] == (0, bytes(plain))
    out.append(_ok("built-15-bit-distance-codes", built, exp))
    out.append(_short("text-5000-capacity-4999", z, O.deflate(z), 4999))
    out.append(_short("mix-70001-capacity-two-thirds", z70, O.deflate(z70), 46667))
    cut = z[:len(z) // 2]
    out.append(_error("text-5000-cut-in-mid-block", cut, O.deflate(cut), 5000))
    return out


def _adler_worst():
    """Two outputs of 700,001 bytes of 0xFF and of zeros at odd residues: Adler-32's largest and smallest increments."""
    out = []
    for name, byte, at in (("ff-700001", b"\xff", (3, 9)), ("zeros-700001", b"\x00", (13, 7))):
        z = corpus.deflate_raw(byte * 700001)
        out.append(_ok(name, z, O.deflate(z), at=at))
    return out


# ----------------------------------------------------------------------------------------------------------------------------- LZ4
LZ4_SOAK_SEEDS = (2, 1, 5, 9)   # random.Random(seed) draws style 0, 1, 2, 3 first; an end the reference accepts; under 140 KB


def _lz4():
    out = []
    for style, seed in enumerate(LZ4_SOAK_SEEDS):
        assert random.Random(seed).randrange(4) == style
        blk, plain = K.random_lz4_block(random.Random(seed), 20000)
        exp = O.lz4_block(blk)
        assert exp == (0, plain) and len(plain) <= 140000
        out.append(_ok("soak-style-%d" % style, blk, exp, hot=True))
    lits = corpus.p_rand(70000, 41)
    blk = K.sequence(lits)
    out.append(_ok("literals-70000", blk, O.lz4_block(blk), hot=True))
    # 40,000 literals, then matches at offsets 32,769 .. 65,535 (test_gpu_lz4.py: far matches right behind a long literal run)
    rnd = random.Random(77)
    lits = corpus.p_rand(40000, 42)
    plain, blk, first = bytearray(lits), bytearray(), True
    for _ in range(40):
        off = rnd.randrange(32769, min(65535, len(plain)) + 1)
        ml = rnd.choice([4, 5, 8, 19, 64, 300, 2000])
        blk += K.sequence(lits if first else b"", off, ml)
        first = False
        for _k in range(ml):
            plain.append(plain[len(plain) - off])
    tail = corpus.p_rand(12, 5)
    blk += K.sequence(tail)
    plain += tail
    exp = O.lz4_block(bytes(blk))
    assert exp == (0, bytes(plain))
    out.append(_ok("far-matches-behind-40000-literals", bytes(blk), exp))
    for n in (1, 5, 12, 13):
        blk = corpus.lz4_block(corpus.p_text(n, 43))
        out.append(_ok("text-%d" % n, blk, O.lz4_block(blk)))
    # history outside the block: the same block with its prefix somewhere else (the lane decoder) and in front of the output (the chain copier)
    hist = corpus.p_text(5000, 44)
    blk = K.sequence(b"", 4000, 300) + K.sequence(corpus.p_rand(100, 45), 4100, 50) + K.sequence(b"", 450, 900) + K.sequence(corpus.p_rand(13, 46))
    exp = O.lz4_block(blk, hist)
    out.append(_ok("prefix-elsewhere", blk, exp, dictionary=hist))
    out.append(_ok("prefix-adjacent", blk, exp, prefix=hist))
    raw = corpus.p_rand(7001, 47)
    out.append(Case("stored-7001", raw, 7001, 0, raw, 7001, 7001, aux=LZ4_STORED))   # SWC_LZ4_STORED: `in` copied (include/swc_hip.h)
    blk = corpus.lz4_block(corpus.p_text(5000, 48))
    out.append(_short("text-5000-capacity-3000", blk, O.lz4_block(blk), 3000))
    bad = K.sequence(corpus.p_rand(20, 49), 5, 10) + K.sequence(corpus.p_rand(4, 50))   # four literals at the end: LZ4.swift:370-372
    out.append(_error("end-the-reference-refuses", bad, O.lz4_block(bad), 64))
    return out


# ------------------------------------------------------------------------------------------------------------------ LZMA2 and LZMA
def _lzma():
    out = []
    sizes = (0, 1, 100, 5000, 70000)
    valid = S.lzma2_valid(sizes=sizes)           # kind (text, rep, zero, rand, mix) x size x dictionary (4 KiB, 64 KiB, 1 MiB)
    assert len(valid) == 75
    for kind in (0, 4):                          # text and mix at every size, 64 KiB dictionary; 70,000 also at 4 KiB
        for s in range(5):
            for d in ((1, 0) if s == 4 else (1,)):
                z, db, x = valid[(kind * 5 + s) * 3 + d]
                assert len(x) == sizes[s]
                out.append(_ok("lzma2-valid-%d-%d" % (len(x), len(out)), z, O.lzma2(z, db), codec="lzma2", aux=db))
    alone = [(z, x) for z, x in S.lzma_alone_valid() if len(x) <= 5000][::3]
    assert len(alone) >= 6
    for k, (z, x) in enumerate(alone):
        b = z[0]
        props = (b % 9, (b // 9) % 5, (b // 9) // 5)
        ds, size = int.from_bytes(z[1:5], "little"), int.from_bytes(z[5:13], "little", signed=True)
        exp = O.lzma_raw(z[13:], props[0], props[1], props[2], ds, size)
        assert exp[:2] == (0, x)
        out.append(_ok("lzma-alone-%d-%d" % (len(x), k), z[13:], exp, codec="lzma", aux=props[0] | props[1] << 8 | props[2] << 16,
                       extra=size & 0xFFFFFFFFFFFFFFFF, dict_value=ds, lzma=props + (ds, size)))
    for shape in ((8, 4, 4), (6, 0, 2)):          # lc + lp > 4: the literal coders live in the workspace (tests/_lzma_build.py)
        c = LB._model_shape("lzma2", shape, collections.Counter())
        exp = O.lzma2(c.stream, c.dict_byte)
        assert c.status == 0 and exp[:2] == (0, c.plain)
        out.append(_ok(c.name, c.stream, exp, codec="lzma2", aux=c.dict_byte))
    z, db, _ = [v for v in S.lzma2_valid(sizes=(5000,)) if v[1] == corpus.lzma2_dict_byte(1 << 16)][0]
    cut = z[:len(z) // 2]
    out.append(_error("lzma2-truncated", cut, O.lzma2(cut, db), 5000, codec="lzma2", aux=db))
    return out


# --------------------------------------------------------------------------------------------------------------------------- BZip2
BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090


def _i32(v):
    return v - (1 << 32) if v & 0x80000000 else v


def _find_magics(stream, magic):
    """Bit offsets of a 48-bit magic (the blocks of a libbz2 stream; its streams here hold none by accident: asserted by the caller)."""
    v, total = int.from_bytes(stream, "big"), len(stream) * 8
    found = []
    for sh in range(8):
        b = ((v << sh) & ((1 << total) - 1)).to_bytes(len(stream), "big")
        at = b.find(magic.to_bytes(6, "big"))
        while at >= 0:
            found.append(at * 8 + sh)
            at = b.find(magic.to_bytes(6, "big"), at + 1)
    return sorted(found)


def _bits(stream, lo, hi):
    v = int.from_bytes(stream, "big")
    return (v >> (len(stream) * 8 - hi)) & ((1 << (hi - lo)) - 1)


def bzip2_blocks(stream):
    """[(bit offset of the block body, stored CRC, the block as a stream of its own, bit offset just behind the block)] of a libbz2
    stream."""
    starts, end = _find_magics(stream, BLOCK_MAGIC), _find_magics(stream, END_MAGIC)
    assert len(end) == 1 and all(s < end[0] for s in starts)
    out = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else end[0]
        crc = _bits(stream, s + 48, s + 80)
        nbits = 32 + (e - s) + 48 + 32
        v = (int.from_bytes(stream[:4], "big") << (nbits - 32)) | (_bits(stream, s, e) << 80) | (END_MAGIC << 32) | crc
        pad = -nbits % 8
        out.append((s + 80, crc, (v << pad).to_bytes((nbits + pad) // 8, "big"), e))
    return out


def _bzip2():
    out = []
    for kind in ("text", "mix"):
        for n in (1, 300, 4000, 79999, 250000):
            x = corpus.PAYLOADS[kind](n, 51)
            z = bz2.compress(x, 1)
            blocks = bzip2_blocks(z)
            whole = b""
            for k, (body, crc, alone, end) in enumerate(blocks):
                exp = O.bzip2(alone)
                assert exp[0] == 0
                whole += exp[1]
                c = _ok("%s-%d-block-%d" % (kind, n, k), z, exp, extra=body, dict_value=crc, hot=True, aux_out=_i32(O.bzip2crc32(exp[1])))
                c.in_consumed = end       # in BITS: where the next magic starts (include/swc_hip.h)
                assert crc == O.bzip2crc32(exp[1])
                out.append(c)
            assert whole == x and (len(blocks) >= 3) == (n == 250000)
    # two blocks built symbol by symbol (tests/_bzip2_build.py): runs over three byte values, and all 258 symbols at 20 bits
    n = collections.Counter()
    for c in (BB.of_text("runs-over-three-byte-values", BB.text_over([0, 0x42, 0x43], 3000, 21, runs=True), n),
              BB.of_text("all-258-symbols-at-20-bits", BB.text_over(list(range(256)), 700, 20), n, tables=[[20] * 258, [20] * 258], odd=True)):
        assert c.status == 0 and len(c.block_bits) == 1
        exp = O.bzip2(c.stream)
        assert exp[:2] == (0, c.plain)
        d = _ok(c.name, c.stream, exp, extra=c.block_bits[0], dict_value=c.block_crc[0], aux_out=_i32(O.bzip2crc32(exp[1])))
        d.in_consumed = None              # (the builder does not say where its block ends)
        out.append(d)
    x = corpus.p_text(4000, 52)
    z = bytearray(bz2.compress(x, 1))
    z[13] ^= 1                                        # the stored CRC of the block
    exp = O.bzip2(bytes(z))
    assert exp[:2] == (210, x)                        # wrongCRC carries the bytes
    out.append(_error("wrong-stored-crc", bytes(z), exp, 4000, extra=112, dict_value=int.from_bytes(z[10:14], "big"), aux_out=_i32(O.bzip2crc32(x))))
    return out


# --------------------------------------------------------------------------------------------------------------------------- Delta
def _delta():
    """(cases out of place, cases in place): every distance x every length; job t of the first list stands at the residue pair
    (t // 16, t % 16) -- all 256 -- and job t of the second at residue t % 16."""
    units = []
    for dist in (1, 2, 3, 4, 7, 255, 0):
        for n in (0, 1, 255, 256, 257, 5000):
            x = corpus.p_rand(n, 60 + dist)
            want = C.create_string_buffer(max(n, 1))
            O.lib.refcpu_delta_decode(x, n, dist, C.cast(want, C.c_void_p))
            units.append((dist, x, want.raw[:n]))
    apart = [Case("distance-%d-length-%d" % (units[t % 42][0], len(units[t % 42][1])), units[t % 42][1], max(len(units[t % 42][1]), 1), 0,
                  units[t % 42][2], len(units[t % 42][1]), None, aux=units[t % 42][0], at=(t // 16, t % 16)) for t in range(256)]
    in_place = [Case("in-place-distance-%d-length-%d" % (units[t % 42][0], len(units[t % 42][1])), units[t % 42][1], max(len(units[t % 42][1]), 1), 0,
                     units[t % 42][2], len(units[t % 42][1]), None, aux=units[t % 42][0], at=((t * 5 + t // 42) % 16,) * 2, in_place=True) for t in range(84)]
    return apart, in_place


# ------------------------------------------------------------------------------------------------------------------------ Encoders
def _encoder_payloads():
    return [corpus.p_text(n, 70 + k) for k, n in enumerate((0, 1, 13, 300, 65536))] + [corpus.p_mix(65537, 76), corpus.p_rand(20000, 77)]


def _encoders():
    """{codec: cases}: status 0, the bytes unknown (data None) -- the test decodes them with the oracle.  out_cap is exactly the
    bound of include/swc_hip.h."""
    groups = {"lz4_compress": [], "deflate_compress": [], "deflate_compress_dynamic": []}
    prefix = corpus.p_text(3000, 78)
    for k, p in enumerate(_encoder_payloads()):
        groups["lz4_compress"].append(Case("lz4-%d" % len(p), p, len(p) + len(p) // 255 + 16, 0, None, None, len(p), source=(b"", p)))
        q = prefix[:1500] + p[:len(p) // 2] + prefix[1500:]       # a block that finds matches in its prefix
        groups["lz4_compress"].append(Case("lz4-prefix-%d" % len(q), prefix + q, len(q) + len(q) // 255 + 16, 0, None, None, None,
                                           extra=len(prefix), source=(prefix, q)))
        for codec in ("deflate_compress", "deflate_compress_dynamic"):
            groups[codec].append(Case("%s-%d" % (codec, len(p)), p, len(p) + len(p) // 8 + 32, 0, None, None, len(p), source=(b"", p)))
    return groups


DEFLATE = _deflate()
ADLER = _adler_worst()
LZ4 = _lz4()
LZMA = _lzma()
BZIP2 = _bzip2()
DELTA, DELTA_IN_PLACE = _delta()
ENCODERS = _encoders()

ERROR_CASES = {"text-5000-cut-in-mid-block", "end-the-reference-refuses", "lzma2-truncated", "wrong-stored-crc"}
for _c in DEFLATE + ADLER + LZ4 + LZMA + BZIP2 + DELTA + DELTA_IN_PLACE + [c for g in ENCODERS.values() for c in g]:
    assert _c.error == (_c.name in ERROR_CASES), _c.name            # status 0 under the oracle everywhere else (_ok, _short)
    assert _c.error == (_c.status not in (0, 901)), _c.name


def check_encoded(codec, case, produced):
    """What an encoder left decodes to its input under the oracle's decoder, which consumes all of it."""
    prefix, block = case.source
    if codec == "lz4_compress":
        assert O.lz4_block(produced, prefix or None) == (0, block), case.name    # (a block decodes whole or not at all)
    else:
        assert O.deflate(produced) == (0, block, len(produced)), case.name


# ---------------------------------------------------------------------------------------------------------------------- placements
def placements(cases, seed, hot=True, per_case=4):
    """[(case index, input residue, output residue)]: the full cross for the hot cases (hot=False: `per_case` pairs like the rest),
    the case's own pair where it names one, else `per_case` pairs of a fixed seeded pairing -- the residues of either side drawn
    from shuffled decks of 0..15, so that sixteen draws in a row cover the set."""
    rnd = random.Random(seed)
    decks = ([], [])

    def draw(side):
        if not decks[side]:
            decks[side].extend(rnd.sample(range(16), 16))
        return decks[side].pop()

    out = []
    for k, c in enumerate(cases):
        if c.at is not None:
            out.append((k, c.at[0], c.at[1]))
        elif c.hot and hot:
            out.extend((k, i, o) for i in range(16) for o in range(16))
        else:
            out.extend((k, draw(0), draw(1)) for _ in range(per_case))
    return out


def encoder_placements(cases, deflate):
    """Every unit at (0, 0) and at the 16 input residues, the outputs at all 16 residues (LZ4) or at 0, 4, 8, 12 (the Deflate
    encoders: the header's rule)."""
    out = []
    for k in range(len(cases)):
        out.append((k, 0, 0))
        out.extend((k, r, 4 * ((r + k) % 4) if deflate else (3 * r + k) % 16) for r in range(16))
    return out
