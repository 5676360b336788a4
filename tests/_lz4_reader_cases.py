"""LZ4 blocks that stand on either side of every comparison the block reader makes (LZ4.process(block:_:), reference
Sources/LZ4/LZ4.swift:332-413), built sequence by sequence (_lz4_build) for the two restatements of that reader: the lane decoder
(csrc/lz4_lane.h, every job whose dictionary is not in place -- group A) and the wave parser (csrc/lz4_wave.h: the checked step
and the sub-chunk rounds, everything else -- group B).  Both tiers run them: test_lz4_reader_emulation.py, test_gpu_lz4_reader.py.
TEST INFRASTRUCTURE ONLY.

A case: name, block, where its history is (`history`: "none", "dict" -- a dictionary somewhere else --, "prefix" -- bytes in place
in front of the output --, "linked" -- the output of a predecessor block of plain literals), the history's bytes (`hist`), the
capacity, and the status the job must end with -- STATED BY HAND from the Swift lines, never taken from the oracle or the engine.
What the block decodes to is the oracle's to say (expected())."""
from collections import namedtuple

import _lz4_build as LB
import _lz4_linked_cases as K
import _oracle as O
from swcompression_amd import corpus

OK, TRUNCATED, CORRUPTED, CAPACITY = K.OK, K.TRUNCATED, K.CORRUPTED, K.CAPACITY

Case = namedtuple("Case", "name block history hist cap status")

DICT_LENGTHS = (1, 3, 11, 12, 65535, 65536, 65537, 70000)
MAX_OFFSET = 65535   # (two bytes: what lies further back in a longer dictionary no offset reaches)
HIST = 300           # group B: the adjacent prefix, the linked predecessor


def _text(n, seed):
    """n bytes of words (never 0xA5, the guard value: a byte read from a guard differs from every byte a case expects)."""
    return corpus.p_text(n, seed)


def _size(seqs, last):
    return sum(len(lit) + ml for lit, _, ml in seqs) + len(last or b"")


# ---- group A: a dictionary somewhere else (the lane decoder) -------------------------------------------------------------------

def _a(out, name, d, seqs, last, status, cap=None, cut=None, slack=0):
    """cap None: exactly what the sequences produce (+ slack)."""
    b = LB.block(seqs, last)
    if cut is not None:
        b = b[:cut]
    out.append(Case("A-d%d-%s" % (len(d), name), b, "dict", d, _size(seqs, last) + slack if cap is None else cap, status))


def _reach_cases(out, d):
    """:382 `offset > 0 && offset <= out.endIndex`: out.endIndex counts the dictionary."""
    n = len(d)
    tail = _text(8, 101)
    for tag, lit in (("at0", b""), ("behind5", _text(5, 102))):
        first = n + len(lit)   # the offset of the dictionary's first byte
        if first <= MAX_OFFSET:
            _a(out, "reach-first-byte-" + tag, d, [(lit, first, 4)], tail, OK)
        else:   # (the first byte is out of any offset's reach: the furthest offset there is)
            _a(out, "reach-65535-" + tag, d, [(lit, MAX_OFFSET, 4)], tail, OK)
        if first + 1 <= MAX_OFFSET:
            _a(out, "reach-one-beyond-" + tag, d, [(lit, first + 1, 4)], tail, CORRUPTED, slack=16)
        _a(out, "offset-0-" + tag, d, [(lit, 0, 4)], tail, CORRUPTED, slack=16)


def _span_cases(out, d):
    """Where a match begins and ends (:406-409): in_dict = offset - position, the bytes of the match that lie in the dictionary."""
    n = len(d)
    lit, tail = _text(3, 103), _text(8, 104)
    for mlen in (4, 9):
        for in_dict, what in ((1, "begins-on-last-dict-byte"), (mlen - 1, "one-byte-into-output"), (mlen, "ends-on-last-dict-byte"),
                              (mlen + 1, "inside-dict")):
            if in_dict <= n:
                _a(out, "span-m%d-%s" % (mlen, what), d, [(lit, len(lit) + in_dict, mlen)], tail, OK)
    if n >= 11:   # far more of the dictionary behind the match's source than the match takes, and room behind the block
        _a(out, "span-deep-inside-dict-roomy", d, [(lit, len(lit) + min(n, 60000), 4)], tail, OK, slack=64)


def _end_rule_cases(out, d):
    n = len(d)
    seven, eight = _text(7, 105), _text(8, 106)
    # :373 `out.endIndex - lastMatchStartIndex >= 12`: both indices count the dictionary.  4 match bytes + 7 literals = 11.
    firsts = [("in-dict" if n >= 4 else "from-dict", [(b"", n if n <= MAX_OFFSET else 40, 4)]), ("crossing", [(b"", 1, 4)]),
              ("behind-3-literals", [(_text(3, 107), 2, 4)])]
    for tag, seqs in firsts:
        _a(out, "rule372-%s-7" % tag, d, seqs, seven, CORRUPTED, slack=16)
        _a(out, "rule372-%s-8" % tag, d, seqs, eight, OK)
    # :371 `literalCount >= 5 || sequenceCount == 1` (8 match bytes + 4 literals = 12: :373 holds)
    one = [(b"ab", 1, 8)]
    _a(out, "rule370-2seq-4", d, one, _text(4, 108), CORRUPTED, slack=16)
    _a(out, "rule370-2seq-5", d, one, _text(5, 109), OK)
    for k in range(5):
        _a(out, "rule370-1seq-%d" % k, d, [], _text(k, 110 + k), OK)
    two = [(b"ab", 1, 8), (b"c", 3, 8)]
    _a(out, "rule370-3seq-4", d, two, _text(4, 108), CORRUPTED, slack=16)
    _a(out, "rule370-3seq-5", d, two, _text(5, 109), OK)


def _truncation_cases(out, d):
    """:344 / :350 / :364 / :378 / :388: the block ends inside a field.  273 literals = 15 + 255 + 3 (two extension bytes), a match
    of 281 = 19 + 255 + 7 (two)."""
    lit = _text(273, 120)
    seqs, tail = [(lit, 1, 281)], _text(8, 121)
    at_lits = 3
    at_offset = at_lits + 273
    for name, cut in (("empty", 0), ("behind-token", 1), ("inside-literal-extension", 2), ("behind-literal-extension", 3),
                      ("inside-literals", at_lits + 100), ("behind-literals", at_offset), ("between-offset-bytes", at_offset + 1),
                      ("behind-offset", at_offset + 2), ("inside-match-extension", at_offset + 3)):
        # (behind the literals the block is not truncated: it IS a block of one sequence, :369)
        _a(out, "cut-" + name, d, seqs, tail, OK if name == "behind-literals" else TRUNCATED, cap=1024, cut=cut)
    b = LB.block(seqs, tail)
    _a(out, "cut-behind-match", d, seqs, tail, TRUNCATED, cap=1024, cut=len(b) - 9)        # :344: no token
    _a(out, "cut-inside-closing-literals", d, seqs, tail, TRUNCATED, cap=1024, cut=len(b) - 1)


def _capacity_cases(out, d):
    lit, tail = _text(5, 130), _text(8, 131)
    for tag, off in (("crossing", 6), ("in-output", 4)):
        seqs = [(lit, off, 7)]
        _a(out, "cap-exact-" + tag, d, seqs, tail, OK)
        _a(out, "cap-one-below-" + tag, d, seqs, tail, CAPACITY, slack=-1)
    # The lane decoder moves eight bytes per step: the room behind a sequence's literals in the output (cap - pos - lit) and in the
    # block (n - ip - lit), and behind a match (cap - p - rem), at the values where an eight-byte step just does not fit, just fits,
    # and fits with a byte to spare -- whatever it moves, it writes nothing behind the sequence and reads nothing behind the block.
    # cap - pos - lit of a sequence that is not the last: what follows it is a match (>= 4) and the closing literals, 12 between them
    # (:373) -- at 7, 8 and 9 the capacity is too small.
    for k in (7, 8, 9):
        _a(out, "cap-literals-room-%d" % k, d, [(lit, 3, 4)], tail, CAPACITY, cap=len(lit) + k)
    # n - ip - lit of a sequence that is not the last: offset (2), the closing token (1) and its literals -- 5 of them (8), 6 (9); with
    # 4 (7) the block breaks :371.
    for k, st in ((4, CORRUPTED), (5, OK), (6, OK)):
        _a(out, "input-room-%d" % (3 + k), d, [(_text(9, 132), 2, 8)], _text(k, 133), st, slack=16 if st else 0)
    # cap - p - rem of a match that 5 closing literals follow: the capacity holds them at 7, 8 and 9
    for k in (7, 8, 9):
        for tag, seqs in (("offset3", [(lit, 3, 9)]), ("offset8", [(_text(8, 134), 8, 9)]), ("offset12", [(_text(12, 135), 12, 9)]),
                          ("crossing-offset3", [(b"ab", 3, 9)]), ("crossing-offset9", [(_text(8, 134), 9, 9)])):
            _a(out, "cap-match-room-%d-%s" % (k, tag), d, seqs, _text(5, 136), OK, slack=k - 5)


def _crossing_cases(out, d):
    """A match that starts in the dictionary and goes on in the output: behind the crossing its source is out[0...], `offset` bytes in
    front of where it writes -- the pattern-replication path for offsets below 8 (`rem` bytes left: below 8, 8, more), the plain
    eight-byte loop from 8 on.  in_dict is the smallest that makes a match of 4 (`few`), or the whole offset (`all`: no literals)."""
    tail = _text(8, 140)
    for off in range(1, 10):
        for rem in range(1, 21):
            for tag, in_dict in (("few", max(1, 4 - rem)), ("all", off)):
                if in_dict > off or in_dict > len(d) or in_dict + rem < 4 or (tag == "all" and in_dict == max(1, 4 - rem)):
                    continue   # (a match of fewer than 4 bytes does not exist: offset 1 leaves at least 3 behind the crossing)
                lit = _text(off - in_dict, 141)
                _a(out, "cross-off%d-rem%d-%s" % (off, rem, tag), d, [(lit, off, in_dict + rem)], tail, OK)
                if rem in (7, 8, 9):   # ... and with room to spare behind the block: the capacity is not what picks the path
                    _a(out, "cross-off%d-rem%d-%s-roomy" % (off, rem, tag), d, [(lit, off, in_dict + rem)], tail, OK, slack=13)


def group_a():
    out = []
    for n in DICT_LENGTHS:
        d = _text(n, 900 + n % 97)
        _reach_cases(out, d)
        _span_cases(out, d)
        _end_rule_cases(out, d)
        _truncation_cases(out, d)
        _capacity_cases(out, d)
        if n == 12:
            _crossing_cases(out, d)
    return out


# ---- group B: no history, an adjacent prefix, a linked predecessor (the wave parser) -------------------------------------------

def _b(out, name, history, seqs, last, status):
    hist = b"" if history == "none" else _text(HIST, 200)
    out.append(Case("B-%s-%s" % (history, name), LB.block(seqs, last), history, hist, 2048, status))


def _probe_blocks(hist_len):
    """(name, sequences, status): about 1 KiB of short sequences -- 11 bytes each, so a round of the parse (n - ip >= 128) takes
    them -- with ONE sequence whose offset is the whole history and everything produced in front of its match (:382, OK), or one
    more (CORRUPTED): the block's first sequence (sub-chunk 0, lane 0), or one that starts 340 bytes into the block (sub-chunk 2)."""
    res = []
    for beyond in (0, 1):
        tag = "beyond" if beyond else "exact"
        res.append(("reach-%s-chunk0" % tag, [(_text(10, 201), hist_len + 10 + beyond, 8)] + K._filler(90, 202), CORRUPTED if beyond else OK))
        front = [(_text(12, 203), 12, 6)] + K._filler(30, 204)
        assert len(LB.block(front, None)) >= 256
        produced = _size(front, b"") + 8
        res.append(("reach-%s-chunk2" % tag, front + [(_text(8, 205), hist_len + produced + beyond, 6)] + K._filler(60, 206),
                    CORRUPTED if beyond else OK))
    return res


def group_b():
    out = []
    for history in ("none", "prefix", "linked"):
        for name, seqs, status in _probe_blocks(0 if history == "none" else HIST):
            _b(out, name, history, seqs, _text(12, 207), status)
        # the end-of-block rules behind sequences the rounds have taken
        front = [(_text(12, 203), 12, 6)] + K._filler(90, 208)
        _b(out, "rule372-7", history, front + [(b"", 12, 4)], _text(7, 105), CORRUPTED)
        _b(out, "rule372-8", history, front + [(b"", 12, 4)], _text(8, 106), OK)
        _b(out, "rule370-4", history, front + [(b"ab", 12, 8)], _text(4, 108), CORRUPTED)
        _b(out, "rule370-5", history, front + [(b"ab", 12, 8)], _text(5, 109), OK)
        for k in range(5):   # :371 sequenceCount == 1 (the checked step alone)
            _b(out, "rule370-1seq-%d" % k, history, [], _text(k, 110 + k), OK)
    return out


_cache = {}


def all_cases():
    if "all" not in _cache:
        _cache["all"] = group_a() + group_b()
        names = [c.name for c in _cache["all"]]
        assert len(set(names)) == len(names)
    return _cache["all"]


def chain_of(c):
    """A case whose history is not a dictionary somewhere else, as a chain of _lz4_linked_cases; the case's block is the last job."""
    assert c.history != "dict"
    if c.history == "linked":
        return K.chain(c.name, [K.J(LB.block([], c.hist), len(c.hist)), K.J(c.block, c.cap, K.LINKED)])
    return K.chain(c.name, [K.J(c.block, c.cap)], prefix=c.hist if c.history == "prefix" else b"")


def oracle_raw(c):
    """What the oracle says of the case: (status, bytes, out_len or None) of its block; for a linked case the chain walk of
    _lz4_linked_cases.expect is the judge."""
    if c.history == "dict":
        st, out = O.lz4_block(c.block, c.hist)
        return st, out, len(out) if st == OK else None
    if c.history == "linked":
        exp = K.expect(chain_of(c))
        assert exp[0] == (OK, c.hist, len(c.hist))
        return exp[1]
    # (K.expect refuses a capacity that is too small; none of these is.  What a job that is not linked leaves of a block that fails,
    # the contract does not say.)
    st, out, n = K.expect(chain_of(c))[0]
    return st, out, n if st == OK else None


def expected(c):
    """(status, bytes, out_len or None) for the job of the case: the oracle's answer, and SWC_E_CAPACITY with the oracle's length and
    bytes where the case's capacity is below what the oracle produced.  Computed once per case."""
    exp = _cache.setdefault("expected", {})
    if c.name not in exp:
        st, out, n = oracle_raw(c)
        if st == OK and len(out) > c.cap:
            st = CAPACITY
        exp[c.name] = (st, out, n)
    return exp[c.name]


def verdict(c, status, out_len, in_consumed, data):
    """What both tiers assert of the case's job: `data` = the first min(out_len, cap) bytes of its output."""
    st, out, n = expected(c)
    assert st == c.status, "%s: the oracle says %d, the case %d" % (c.name, st, c.status)
    assert status == st, "%s: status %d, expected %d" % (c.name, status, st)
    if st == OK:
        assert out_len == len(out) and data == out, c.name + ": bytes"
        assert in_consumed == len(c.block), c.name + ": in_consumed"
    elif st == CAPACITY:
        assert out_len == len(out), c.name + ": out_len is not the size the block needs"
        assert data == out[:c.cap], c.name + ": the bytes below the capacity"
    elif n is not None:
        assert out_len == n, c.name + ": out_len"


def frame_of(block):
    """The block as the only one of a frame of independent blocks (64 KiB maximum), no checksums but the header's."""
    import struct
    desc = bytes([0x60, 0x40])
    return struct.pack("<I", 0x184D2204) + desc + bytes([(O.xxh32(desc) >> 8) & 0xFF]) + struct.pack("<I", len(block)) + block + struct.pack("<I", 0)
