"""PAIR entries of the direct lit/len table (csrc/inflate_sync.h) on the host emulation: what every entry of a built table yields
against a scalar decode of its index, directed streams against the oracle, and phase 1 byte for byte against the same sources
built with -DSWC_SYNC_NO_PAIRS=1 (the entry format without pairs)."""
import random
import zlib

import pytest

import _deflate_build as B
import _deflate_pairs_cases as PC
import _emu_deflate_phase1 as P
import _oracle as O

LIT_BITS, DIST_BITS = P.LIT_BITS, P.DIST_BITS
PAIR_LEN_MAX = 127   # kPairLenMax: the length field of a pair entry has seven bits


@pytest.fixture(params=[0, 1, 2], ids=["forward", "reverse", "shuffled"])
def order(request):
    P.set_order(request.param)
    yield request.param
    P.set_order(0)


@pytest.fixture(params=[0, 1], ids=["one-wave", "team"])
def team(request):
    P.set_team(request.param)
    yield request.param
    P.set_team(0)


# ---------------------------------------------------------------------------------------------- the tables
def _by_prefix(lengths):
    """[(code with its bits reversed, length, symbol)] of a set that is not over-subscribed"""
    return [(B._reverse(c, n), n, s) for s, (c, n) in B._ref_codes(list(lengths)).items()]


def _find(codes, idx, width):
    """The symbol whose code the `width` index bits begin with, ("link",) if they are the first bits of a longer code, else None."""
    for rev, n, s in codes:
        if n <= width and rev == idx & ((1 << n) - 1):
            return s, n
    for rev, n, s in codes:
        if n > width and (rev ^ idx) & ((1 << width) - 1) == 0:
            return ("link",)
    return None


def _ref_dist(dcodes, idx, width=DIST_BITS):
    got = _find(dcodes, idx, width)
    if got is None or (got != ("link",) and got[0] > 29):
        return ("stop",)
    if got == ("link",):
        return got
    s, n = got
    return ("dist", n + B.DIST_BITS[s], B.DIST_BASE[s] + ((idx >> n) & ((1 << B.DIST_BITS[s]) - 1)), "lit", 1)


def _ref_lit(lcodes, dcodes, idx, pairs):
    """What a step at index bits `idx` (the bits behind them zero) yields: kind, bits taken, value(s), the table of the next step, toggle"""
    got = _find(lcodes, idx, LIT_BITS)
    if got is None or (got != ("link",) and got[0] > 285):
        return ("stop",)
    if got == ("link",):
        return got
    s, n = got
    if s < 256:
        return ("lit", n, s, "lit", 0)
    if s == 256:
        return ("eob", n)
    e = B.LEN_BITS[s - 257]
    length = B.LEN_BASE[s - 257] + ((idx >> n) & ((1 << e) - 1))
    r = LIT_BITS - n - e
    if pairs and r > 0 and length <= PAIR_LEN_MAX:
        # the rule: the r index bits left address the direct distance table; a plain distance symbol of at most r bits pairs
        d = _find(dcodes, (idx >> (n + e)) & ((1 << DIST_BITS) - 1), min(r, DIST_BITS))
        if d is not None and d != ("link",) and d[0] <= 29:
            ds, dn = d
            return ("pair", n + e + dn + B.DIST_BITS[ds], length, B.DIST_BASE[ds] + ((idx >> (n + e + dn)) & ((1 << B.DIST_BITS[ds]) - 1)), "lit", 0)
    return ("len", n + e, length, "dist", 1)


def _entry(e, idx, shift, pairs):
    """The same from a table entry.  shift: the index bits in front of the entry's own (0)."""
    n2, c2 = e & 31, (e >> 5) & 31
    if e & 0xC000001F == 0:
        return ("link",)
    if e >> 30 & 1:
        return ("eob", n2 - 2) if n2 > 2 else ("stop",)
    extra = (((idx << 2) & ((1 << n2) - 1)) >> c2)
    pair = pairs and e >> 28 & 1
    if pairs:
        base = ((e >> 14) & (3 if pair else 0x1FF)) << (e >> 23 & 15)
        assert e >> 27 & 1 == 0
    else:
        base = e >> 14 & 0x7FFF
    is_len, is_lit, is_dist, tog = e >> (LIT_BITS + 2) & 1, e >> 13 & 1, e >> 29 & 1, e >> 31
    notlen = e >> (DIST_BITS + 2) & ((1 << (LIT_BITS - DIST_BITS)) - 1)
    assert notlen == (0 if is_len else (1 << (LIT_BITS - DIST_BITS)) - 1), "the table switch bits"
    nxt = "dist" if is_len else "lit"
    if pair:
        assert is_dist and not is_lit and not is_len
        return ("pair", n2 - 2, e >> 16 & 127, base + 1 + extra, nxt, tog)
    assert is_len + is_lit + is_dist == 1
    if is_lit:
        return ("lit", n2 - 2, base, nxt, tog)
    if is_len:
        return ("len", n2 - 2, base + extra, nxt, tog)
    return ("dist", n2 - 2, base + 1 + extra, nxt, tog)


def _check_tables(lit, dist, what):
    """Every direct entry of both builds against the scalar decode; returns the number of pair entries."""
    lcodes, dcodes = _by_prefix(lit), _by_prefix(dist)
    n_pairs = 0
    for lib, pairs in ((P.shipped, True), (P.plain, False)):
        fast, ltab, dtab = P.tables(lib, lit, dist)
        assert fast, what   # (no set here is over-subscribed or deeper than the subtables hold)
        for idx in range(1 << DIST_BITS):
            assert _entry(dtab[idx], idx, 0, pairs) == _ref_dist(dcodes, idx), "%s: distance index %d (pairs %d)" % (what, idx, pairs)
        for idx in range(1 << LIT_BITS):
            want = _ref_lit(lcodes, dcodes, idx, pairs)
            assert _entry(ltab[idx], idx, 0, pairs) == want, "%s: lit/len index %d (pairs %d)" % (what, idx, pairs)
            n_pairs += want[0] == "pair"
    return n_pairs


def _vec(d, n):
    return B.vector(d, n)


DIRECTED_SETS = {
    # (lit lengths, distance lengths, pairs expected: True some, False none)
    "pair-of-exactly-the-index-bits-and-one-more": (_vec(PC.fill_complete({257: 5, 258: 6, 256: 2}, [97, 98, 99, 100, 101]), 286), [5, 5, 5, 5], True),
    "length-extra-bits-inside-the-index": (_vec(PC.fill_complete({265: 3, 269: 3, 273: 4, 256: 4}, [97, 98, 99, 100]), 286), [2, 2, 3, 3, 3], True),
    "one-distance-code-of-one-bit": (PC.LIT_V, [1], True),
    "distance-tree-with-an-unused-code": (PC.LIT_V, [1, 2], True),
    "distance-symbols-30-31-behind-a-short-length": (_vec(PC.fill_complete({257: 2, 256: 2}, [97, 98]), 286), [1] + [0] * 29 + [2, 2], True),
    "length-symbols-286-287": (_vec(PC.fill_complete({286: 3, 287: 3, 257: 3, 256: 3}, [97, 98]), 288), PC.DIST_V, True),
    "distance-link-behind-a-one-bit-length": (_vec({257: 1, 97: 2, 256: 2}, 286), [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10], True),
    "lengths-beyond-the-pair-field": (_vec(PC.fill_complete({285: 2, 281: 3, 256: 3}, [97, 98, 99]), 286), [1, 1], False),
    "fixed-codes": (B.FIXED_LIT, B.FIXED_DIST, False),
    "the-case-streams-sets": (PC.LIT_V, PC.DIST_V, True),
}


@pytest.mark.parametrize("name", sorted(DIRECTED_SETS))
def test_directed_code_sets_entry_by_entry(name):
    lit, dist, some = DIRECTED_SETS[name]
    n = _check_tables(lit, dist, name)
    assert (n > 0) == some, "%s: %d pair entries" % (name, n)


def test_directed_sets_hold_what_they_were_built_for():
    lit, dist, _ = DIRECTED_SETS["pair-of-exactly-the-index-bits-and-one-more"]
    lc, dc = _by_prefix(lit), _by_prefix(dist)
    kinds = {s: {_ref_lit(lc, dc, i, True)[0] for i in range(1 << LIT_BITS) if _find(lc, i, LIT_BITS) == (s, lit[s])} for s in (257, 258)}
    assert kinds == {257: {"pair", "len"}, 258: {"len"}}   # 5 + 5 bits pair (the four codes there are), 6 + 5 never do
    lit, dist, _ = DIRECTED_SETS["distance-link-behind-a-one-bit-length"]
    lc, dc = _by_prefix(lit), _by_prefix(dist)
    got = {_ref_lit(lc, dc, i, True)[0] for i in range(1 << LIT_BITS) if i & 1 == B._reverse(B._ref_codes(lit)[257][0], 1)}
    assert got == {"pair", "len"}                          # distance codes of up to 8 bits pair, the links behind 9 and 10 do not
    _, ltab, _ = P.tables(P.shipped, lit, dist)
    assert max((e & 31) - 2 for e in ltab if e >> 28 & 1 and e >> 30 & 1 == 0) <= LIT_BITS + 13


@pytest.mark.parametrize("seed", range(4))
def test_random_code_sets_entry_by_entry(seed):
    """200 seeded sets in all: complete ones of every depth, with and without long codes, and incomplete distance sets."""
    rnd = random.Random(0x9A1250 + seed)
    total = 0
    for k in range(50):
        nlit = rnd.choice([3, 10, 40, 120, 256])
        nlen = rnd.choice([1, 2, 5, 12, 29])
        lsyms = rnd.sample(range(256), nlit) + [256] + rnd.sample(range(257, 286), nlen)
        lit = B.random_complete_lengths(rnd, lsyms, max(rnd.choice([6, 9, 11, 15]), len(lsyms).bit_length()), rnd.choice([0.0, 0.3, 0.9]))
        dsyms = rnd.sample(range(30), rnd.choice([1, 2, 4, 10, 30]))
        dist = B.random_complete_lengths(rnd, dsyms, max(rnd.choice([3, 5, 9, 15]), len(dsyms).bit_length()), rnd.choice([0.0, 0.5, 0.95]))
        if rnd.randrange(4) == 0 and len(dist) > 2:
            del dist[rnd.choice(sorted(dist))]          # an unused code
        total += _check_tables(B.vector(lit, 286), B.vector(dist, 30), "seed %d set %d" % (seed, k))
    assert total > 0


# ---------------------------------------------------------------------------------------------- the streams
def _expectations():
    cases = PC.directed()
    exp = []
    for name, z, cap in cases:
        st, out, cons = O.deflate(z)
        exp.append((st, out, cons))
    return cases, exp


CASES, EXPECTED = _expectations()
_BY_NAME = {c[0]: e for c, e in zip(CASES, EXPECTED)}
assert all(_BY_NAME["pair-distance-one-beyond-the-output-at-%d" % at][0] == PC.E_TRAP for at in (0, 1, 32767))
assert all(_BY_NAME["pair-distance-exactly-the-output-at-%d" % at][0] == 0 for at in (1, 32767))
assert all(e[0] == PC.E_NOT_FOUND for n, e in _BY_NAME.items() if n.startswith("input-ends-"))
assert all(e[0] == 0 for n, e in _BY_NAME.items() if not n.startswith(("input-ends-", "pair-distance-one-beyond")))
assert len(_BY_NAME["4096-pairs-and-nothing-else"][1]) > 4096 * 3


def test_the_case_streams_are_made_of_pairs():
    """The streams mean what their names say: with the case sets every match token of them is one direct entry."""
    lc, dc = _by_prefix(PC.LIT_V), _by_prefix(PC.DIST_V)
    for tok in (PC.PAIR, PC.LONG_PAIR, PC.MATCH, ("sym", 264, 0, 4, 0), ("sym", 258, 0, 29, 8191), ("sym", 258, 0, 0, 0)):
        w = B.BitWriter()
        B._write_tokens(w, [tok], B._reversed_codes(PC.LIT_V), B._reversed_codes(PC.DIST_V), False)
        bits = int.from_bytes(w.data(), "little")
        got = _ref_lit(lc, dc, bits & ((1 << LIT_BITS) - 1), True)
        assert got[0] == "pair" and got[1] == w.bit_length() and got[2] == B.LEN_BASE[tok[1] - 257] + tok[2], tok


def test_directed_streams_against_the_oracle(order, team):
    caps = [cap if cap is not None else max(len(e[1]), 1) for (_, _, cap), e in zip(CASES, EXPECTED)]
    res = P.inflate(P.shipped, [z for _, z, _ in CASES], caps)
    ref = P.inflate(P.plain, [z for _, z, _ in CASES], caps)
    for (name, _, cap), e, r, q in zip(CASES, EXPECTED, res, ref):
        st, out, cons, n = r
        assert r == q, "%s: not what the format without pairs gives" % name
        if cap is not None and cap < len(e[1]):
            assert st == PC.E_CAPACITY and n == len(e[1]) and out == e[1][:cap], "%s: capacity" % name
            continue
        assert st == e[0], "%s: status %d, oracle %d" % (name, st, e[0])
        if e[0] == 0:
            assert out == e[1] and cons == e[2] and n == len(e[1]), "%s: bytes / in_consumed / out_len" % name


def test_directed_streams_phase_1_is_the_one_without_pairs(order, team):
    for name, z, cap in CASES:
        cap = cap if cap is not None else max(len(_BY_NAME[name][1]), 1)
        for aux in (0, 1 | 4):          # alone; SWC_DEFLATE_JOINED | SWC_DEFLATE_LINKED: distances may reach into a history
            assert P.phase1(P.shipped, z, cap, aux, team) == P.phase1(P.plain, z, cap, aux, team), (name, aux)


def test_linked_unit_pair_reaches_into_its_history(team):
    """A linked unit takes 32,768 bytes of history for granted and notes how far it reached (the copy has the last word): a pair
    at positions 0 and 1 whose distance goes 1 and 32,768 - position bytes in front of the unit.  This is the test that guards
    the ORDER of the pair step -- `need` takes distance - nout BEFORE nout grows by the length: the reach it pins is exact.  The
    trap streams of the directed cases (a distance one beyond the output at 0, 1 and 32,767) do not guard it: they
    still pass with `need` taken after `nout` (tried as a mutation)."""
    for at, distance in ((0, 1), (0, 32768), (1, 2), (1, 32768), (1, 1)):
        s = PC.Stream(prefix=0)
        s.header()
        if at:
            s.put(97)
        s.put(("sym", 258, 0) + B._DIST_SYM[distance], 98)
        s.eob()
        got = P.phase1(P.shipped, s.data(), 64, 1 | 4, team)
        assert got == P.phase1(P.plain, s.data(), 64, 1 | 4, team)
        assert got[0] == 0 and got[1] == at + 5 and got[5] == distance - at, (at, distance, got[:7])


def test_linked_unit_pair_exactly_into_and_one_beyond_its_history(order, team):
    """Both phases of a launch with linked units (the emulation of tests/host_emu/emu_deflate_linked.cpp, built from the sources as
    they are): the copy knows the history that came to be -- five bytes -- and has the last word on the pair that reaches for six."""
    import _deflate_linked_cases as L
    import _emu_deflate_linked as EL
    EL.set_order(order)
    try:
        verdicts = {}
        for name, units in PC.linked_runs().items():
            exp = L.expect(units)
            res = EL.run_units(units, arrangement=EL.COPIER, team=team)
            for k, (e, r) in enumerate(zip(exp, res)):
                assert r[0] == e[0] and r[3] == e[3], "%s unit %d: status / aux" % (name, k)
                if e[1] is not None:
                    assert (r[1], r[2]) == (e[1], e[2]), "%s unit %d: out_len / in_consumed" % (name, k)
                if e[4] is not None:
                    assert r[5] == e[4], "%s unit %d: bytes" % (name, k)
            verdicts[name] = (exp[1][0], res[1][6])
        assert verdicts == {"linked-pair-reaches-exactly-into-its-history": (0, 5), "linked-pair-reaches-one-beyond-its-history": (PC.E_TRAP, 6)}
    finally:
        EL.set_order(0)


# ---------------------------------------------------------------------------------------------- equality on zlib's streams
def _spliced(rnd, n):
    from swcompression_amd import corpus
    out = bytearray()
    while len(out) < n:
        kind = rnd.choice(["text", "text", "text", "mix", "bin", "rep"])
        piece = corpus.PAYLOADS[kind](rnd.choice([200, 3000, 20000, 70000]), rnd.randrange(1000))
        at = rnd.randrange(len(piece))
        out += piece[at:at + rnd.randrange(1, 30000)]
    return bytes(out[:n])


@pytest.mark.parametrize("part", range(6))
def test_zlib_streams_phase_1_and_output_equal_the_format_without_pairs(part):
    """300 seeded streams in all (levels 1 / 6 / 9, 200 .. 70,000 bytes): results, stream header, records and literal stream of phase 1
    byte for byte.  For the running time this is weaker than the directed tests: every stream runs in ONE lane order and ONE form
    (one wave, team), which rotate with the stream (k % 3, (k // 3) % 2), not in all six; and both phases with the output compared
    to the text run for every tenth stream only."""
    rnd = random.Random(0xE9A1 + part)
    for k in range(50):
        n = rnd.choice([200, 1000, 5000, 20000, 65536, 70000]) if k % 5 else rnd.randrange(200, 70001)
        text = _spliced(rnd, n)
        c = zlib.compressobj(rnd.choice([1, 6, 9]), zlib.DEFLATED, -15)
        z = c.compress(text) + c.flush()
        P.set_order(k % 3)
        team = (k // 3) % 2
        a, b = P.phase1(P.shipped, z, n, 0, team), P.phase1(P.plain, z, n, 0, team)
        assert a == b, "part %d stream %d: phase 1 differs" % (part, k)
        assert a[:3] == (0, n, len(z))
        if k % 10 == 0:
            P.set_team(team)
            assert P.inflate(P.shipped, [z], [n]) == [(0, text, len(z), n)]
            P.set_team(0)
    P.set_order(0)
