"""CPU tier: the self-check of the LZMA / LZMA2 stream builder (tests/_lzma_build.py).  Before any built stream is compared with
the kernels, the oracle must return exactly what the builder meant -- (0, plain, consumed), or the status an error case was built
for -- liblzma must agree wherever the builder's rule says it can (lc + lp <= 4, a dictionary reset first, properties behind a
dictionary-resetting stored chunk, no end marker inside a chunk, no match across a dictionary reset, a dictionary of 4 KiB or more),
and the builder's counters must show that the directed set reaches what it was written to reach."""
import lzma
import random
import struct

import pytest

import _lzma_build as B
import _oracle as O


def oracle(c):
    """The oracle's (status, bytes, consumed) on a built case; its output cap stays where the rest of the suite keeps it
    (1 GiB: far above the 2 MiB of the largest built stream, so no case can end as 901)."""
    if c.kind == "lzma2":
        return O.lzma2(c.stream, c.dict_byte)
    lc, lp, pb, ds, declared = c.props
    return O.lzma_raw(c.stream, lc, lp, pb, ds, declared)


def liblzma_agrees(c):
    try:
        if c.kind == "lzma2":
            d = lzma.LZMADecompressor(lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": B.lzma2_dict_size(c.dict_byte)}])
            return d.decompress(c.stream) == c.plain and d.eof and d.unused_data == c.stream[c.consumed:]
        lc, lp, pb, ds, declared = c.props
        d = lzma.LZMADecompressor(lzma.FORMAT_ALONE)
        return d.decompress(bytes([(pb * 5 + lp) * 9 + lc]) + struct.pack("<Iq", ds, declared) + c.stream) == c.plain and d.eof
    except lzma.LZMAError:
        return False


def test_range_encoder_against_liblzma_on_plain_literals():
    """The smallest whole: literals only, every byte value, lc 3 / lp 0 / pb 2 -- what the encoder wrote is what liblzma reads."""
    b = B.Builder("lzma", props=(3, 0, 2), dict_size=1 << 16)
    rnd = random.Random(7)
    for _ in range(3000):
        b.literal(rnd.randrange(256))
    b.end_marker()
    c = b.case("literals")
    assert c.liblzma_ok and liblzma_agrees(c) and oracle(c) == (0, c.plain, len(c.stream))


def test_slots_and_lengths_tables():
    for slot in range(64):
        for rem in B.slot_patterns(slot):
            assert B.pos_slot_of(B.slot_base(slot) + rem) == slot
    assert B.slot_base(63) + B.slot_patterns(63)[-1] == 0xFFFFFFFF
    assert [B.lzma2_dict_size(x) for x in (0, 1, 2, 18, 39)] == [4096, 6144, 8192, 1 << 21, 3 << 30]


def test_directed_streams_mean_what_they_were_built_for():
    cases = B.directed_cases()
    assert len(cases) >= 60 and len({c.name for c in cases}) == len(cases)
    for c in cases:
        st, out, cons = oracle(c)
        if c.status == 0:
            assert (st, out, cons) == (0, c.plain, c.consumed), "%s: oracle status %d, %d bytes, %d consumed" % (c.name, st, len(out), cons)
            assert len(c.plain) <= (1 << 21 if c.name == "every-pos-slot-to-2MiB" else 1 << 16), c.name
            if c.liblzma_ok:
                assert liblzma_agrees(c), c.name
        else:
            assert c.plain is None and not c.liblzma_ok and st == c.status, "%s: oracle status %d" % (c.name, st)
    by_name = {c.name: c for c in cases}
    assert by_name["state-11-pos-state-15-long-rep0-traps"].status == 900 and by_name["long-rep-first-behind-a-dictionary-reset"].status == 304
    assert by_name["distance-dict-size"].status == 0 and by_name["distance-dict-size-plus-one"].status == 307
    assert by_name["end-marker-at-exactly-unpack"].status == 0 and by_name["end-marker-before-unpack"].status == 404
    assert by_name["match-reaching-behind-a-dictionary-reset"].status == 0 and not by_name["match-reaching-behind-a-dictionary-reset"].liblzma_ok
    assert by_name["0xA0-first-uses-the-default-properties"].status == 0 and len(by_name["every-pos-slot-to-2MiB"].plain) > 1 << 20
    assert not by_name["0x80-behind-a-stored-chunk-that-reset-the-dictionary"].liblzma_ok and by_name["0x80-behind-a-stored-chunk"].liblzma_ok
    assert by_name["properties-3-to-12-to-3"].status == 0 and by_name["raw-lzma-dictionary-of-1-bytes-end-marker"].status == 0
    assert sum(c.liblzma_ok for c in cases) >= 30      # (liblzma confirms a good part of the set, the oracle all of it)


def test_directed_set_covers_what_it_was_written_for():
    B.directed_cases()
    n = B.directed_counters()
    missing = [(k, s) for k in B.KINDS for s in range(12) if not n["packet", k, s]]
    assert not missing, "packet kind x state never written: %r" % missing
    assert all(n["control", c] for c in (0x80, 0xA0, 0xC0, 0xE0, 1, 2))
    assert all(n["len", coder, tier] for coder in ("len", "rep_len") for tier in ("low", "mid", "high"))
    assert all(n["len-value", coder, v] for coder in ("len", "rep_len") for v in range(2, 274))
    assert all(n["len-pos-state", coder, ps] for coder in ("len", "rep_len") for ps in range(16))
    assert all(n["slot", s] for s in list(range(42)) + [42, 47, 55, 62, 63])      # 0 .. 41: what 2 MiB of output allow
    for lc, lp, pb in B.SHAPES:
        assert n["shape", lc, lp, pb] >= 2                                         # as LZMA2 chunks and as raw LZMA
    assert sum(1 for k in n if k[0] == "coder") > 256                              # (far more literal coders than four cache lines)


@pytest.mark.parametrize("seed", range(3))
def test_random_streams_mean_what_they_were_built_for(seed):
    rnd = random.Random(0x12A4B + seed)
    constructs, kinds = set(), set()
    for i in range(80):
        strict = i % 2 == 0
        c = B.random_stream(rnd, rnd.choice([1, 9, 300, 4000, 20000]), strict, constructs=None if strict else constructs)
        assert oracle(c) == (0, c.plain, c.consumed), (seed, i)
        assert len(c.plain) <= 1 << 16
        if strict:
            assert c.liblzma_ok and liblzma_agrees(c), (seed, i)
        kinds.add((c.kind, strict))
    assert len(kinds) == 4
    # the random set must not shrink to what liblzma would have written
    for construct in ("lc+lp>4", "no properties behind a dictionary-resetting stored chunk", "property change without a dictionary reset",
                      "distance behind a dictionary reset", "end marker in a chunk", "small dictionary"):
        assert construct in constructs, construct
