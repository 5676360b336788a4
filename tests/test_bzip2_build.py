"""CPU tier: the self-check of the BZip2 stream builder (tests/_bzip2_build.py).  Before any built stream is compared with the
kernels, the oracle must return exactly what the builder meant -- (0, plain, consumed), or the status an error case was built for --
libbz2 must agree wherever the builder's rule says it can (prefix-free complete codes of 1 .. 20 bits, at least as many selectors as
groups and at most 18,002, origPtr inside a block that is not empty and not larger than the level allows, no four equal bytes without a
count at the end of a block; like the reference it walks n steps from origPtr whatever the cycles of L), and the builder's counters
must show that the directed set reaches what it was written to reach."""
import bz2
import random

import pytest

import _bzip2_build as B
import _oracle as O
import _streams as S


@pytest.fixture(autouse=True)
def output_cap():
    """The oracle's output cap where the built set expects it (a run of 2^25 is 901 on both sides), and back."""
    O.lib.refcpu_set_max_output(B.MAX_OUTPUT)
    yield
    O.lib.refcpu_set_max_output(1 << 30)


def libbz2_agrees(c):
    try:
        d = bz2.BZ2Decompressor()
        return d.decompress(c.stream) == c.plain and d.eof and d.unused_data == c.stream[c.consumed:]
    except (OSError, ValueError):
        return False


def bits_of(data):
    return bin(int.from_bytes(b"\x01" + data, "big"))[3:]


def occurrences(bits, magic):
    word, at, found = "{:048b}".format(magic), -1, []
    while True:
        at = bits.find(word, at + 1)
        if at < 0:
            return found
        found.append(at)


def test_layers_on_their_own():
    rnd = random.Random(5)
    for n in (1, 2, 5, 64, 700, 4095, 4096, 5000):
        T = bytes(rnd.choice(b"abcd\x00\xff") for _ in range(n))
        L, orig = B.bwt_forward(T)
        assert B.bwt_reverse(L, orig) == T and B.cycles(L) == 1
        used = sorted(set(L))
        assert B.symbols_decode(B.mtf_encode(L, used) + [len(used) + 1], used) == (0, L)
        assert B.bz_crc(T) == S._bzip2_crc(T) == O.bzip2crc32(T)
    assert B.bwt_reverse(b"abc", 3) is None and B.bwt_reverse(b"", 0) == b""
    assert B.rle1_undo(b"aaaa\x02b") == b"aaaaaab" and B.rle1_undo(b"xaaaa") == b"xaaaa" and B.rle1_undo(b"aaaaa") == b"a" * 101 and B.rle1_undo(b"aaaa\x00aaaa") == b"a" * 8
    assert [B.run_digits(r) for r in (1, 2, 3, 4, 7)] == [[0], [1], [0, 0], [1, 0], [0, 0, 0]]
    # 64 digits wrap: RUNB 64 times is -2 and is skipped without a reset, 2^64 + 5 is a run of 5
    assert B.symbols_decode([2] + [1] * 64 + [2, 0, 0, 2, 3], [7, 8]) == (0, bytes([8, 7, 8]))
    assert B.symbols_decode(B.run_digits((1 << 64) + 5) + [2, 3], [7, 8]) == (0, bytes([7] * 5 + [8]))
    assert B.symbols_decode([0, 2], []) == (900, None)
    assert B.ref_codes([1, 2, 3, 0, 3]) == S._ref_codes([1, 2, 3, 0, 3])
    # the bit layer alone against libbz2: a block written field by field
    b = B.Builder(3)
    L, orig = B.bwt_forward(b"mississippi")
    used = sorted(set(L))
    assert used == [0x69, 0x6D, 0x70, 0x73]
    body = b.block_header(B.bz_crc(b"mississippi"), orig, 0, 0x0300, [0x0044, 0x9000])
    b.counts(2, 1)
    b.selectors([1])
    b.table_lengths([2, 2, 2, 3, 4, 4])
    b.table(3, [[], [-1], [], [1], [], [1, -1]])
    b.symbols(B.mtf_encode(L, used) + [5], [[2, 2, 2, 3, 4, 4], [3, 2, 2, 3, 3, 3]], [1])
    b.combined = B.bz_crc(b"mississippi")
    b.end_of_stream()
    assert body == 32 + 80 and bz2.decompress(b.data()) == b"mississippi" and O.bzip2(b.data()) == (0, b"mississippi", len(b.data()))


def test_directed_streams_mean_what_they_were_built_for():
    cases = B.directed_cases()
    assert len(cases) >= 120 and len({c.name for c in cases}) == len(cases)
    built_for_901 = {"one-run-of-2^25"}
    for c in cases:
        st, out, cons = O.bzip2(c.stream)
        assert st == c.status, "%s: oracle status %d, built for %d" % (c.name, st, c.status)
        assert (st == 901) == (c.name in built_for_901), c.name
        if st == 0:
            assert (out, cons) == (c.plain, c.consumed), "%s: %d bytes, %d consumed" % (c.name, len(out), cons)
            if len(c.stream) <= 2000:     # (the restated reference in Python, bit by bit: the small streams)
                assert B.model_stream(c.stream)[:3] == (0, c.plain, c.consumed), c.name
        else:
            assert not c.libbz2_ok
            if st == 210:
                assert out == c.plain, c.name
        if c.libbz2_ok:
            assert libbz2_agrees(c), c.name
    assert sum(c.libbz2_ok for c in cases) * 3 >= len(cases)      # (libbz2 confirms a third of the set, the oracle all of it)
    by = {c.name: c for c in cases}
    # (no symbol map at all: the end-of-block symbol is number 1, which the loop takes for RUNB first -- such a block never ends, it
    # runs out of selectors or of input; usedSymbols[0] of the empty list is never reached)
    for name, st in (("n_used-0-with-a-run", 207), ("n_used-0-with-a-run-to-the-end-of-the-input", 209), ("n_tables-7", 206), ("4-tables-selector-index-4", 207), ("n_selectors-needed-minus-1", 207),
                     ("n_selectors-0", 900), ("eob-as-symbol-51-without-its-selector", 207), ("code-length-start-21", 208),
                     ("non-final-symbol-driven-to--1-in-table-1", 208), ("non-final-symbol-driven-to-0-in-table-1", 0),
                     ("final-symbol-at-26-in-table-1", 0), ("incomplete-code-whose-missing-word-occurs", 209),
                     ("over-subscribed-table-alternating-with-a-prefix-free-one", 0), ("origPtr-40-of-40", 900), ("origPtr-16777215-of-40", 900),
                     ("wrong-crc-on-block-2-of-3", 210), ("wrong-combined-crc", 210), ("one-run-of-2^25", 901), ("one-run-of-2^23", 0),
                     ("BZh1-with-L-of-400100", 0), ("two-cycles", 0), ("run-of-130-digits-wrapped-not-positive", 0)):
        assert by[name].status == st, name
    assert len(by["one-run-of-2^23"].stream) < 100 and len(by["rle1-50000-of-aaaa-ff"].plain) == 2590000
    tails = [c for c in cases if c.name.endswith("behind-the-end-of-stream-magic")]
    assert len(tails) >= 20 and len({c.plain for c in tails}) == 1 and len({len(c.stream) for c in tails}) == len(tails)
    for c in cases:                  # nothing between 2^23 (and the two bytes around that run) and 2^25: the engine's 15 MiB, the oracle's 16
        assert all(l <= (1 << 23) + 2 or l >= 1 << 25 for l in c.l_len) and (c.plain is None or len(c.plain) <= (1 << 23) + 2), c.name


def test_directed_set_covers_what_it_was_written_for():
    cases = B.directed_cases()
    n = B.directed_counters()
    assert all(n["n_used", k] for k in B.N_USED_BOUNDARIES + (0,))
    assert all(n["tables", k] for k in range(8))
    assert all(n["selector", nt, c] for nt in range(2, 7) for c in range(nt + 1))      # (index n_tables: the wrongSelector case)
    assert all(n["position", p] for p in B.LIST_POSITIONS)
    assert all(n["digits", d] for d in range(1, 24)) and all(n["wrapped", d] for d in (63, 64, 65, 66, 130))
    # the placements of a run by name: at the block start and before the end of the block 1 .. 22 digits (23: the block that is
    # nothing but the run of 2^23), split across a table switch 2 .. 18 digits at the first, the middle and the last place
    names = {c.name for c in cases}
    assert all("run-of-%d-digits-%s" % (d, w) in names for d in range(1, 23) for w in ("at-the-block-start", "before-eob"))
    assert all("run-of-%d-digits-split-%d-before-a-table-switch" % (d, s) in names for d in range(2, 19) for s in {1, d // 2, d - 1})
    assert [c.l_len for c in cases if c.name == "one-run-of-2^23"] == [[1 << 23]]
    sides = {}
    for key in n:
        if key[0] == "stage":
            sides.setdefault(key[1:3], set()).add((key[3], key[4]))
    # (i, k): the place of the byte symbol that ends the run in its group, the bytes staged in front of it; (True, 0): the longest run
    # the rule admits there, (False, 1): one more
    both = [ik for ik, s in sides.items() if (True, 0) in s and (False, 1) in s]
    assert len(both) >= 20, sorted(both)
    assert all(n["rle1-cut", s] == 63 for s in ("inside", "count", "behind")) and not n["rle1-cut", "literal"]
    # block starts at each of the 8 bit alignments (second and later blocks), the magics inside block data at each of the 8
    assert {bit % 8 for c in cases for bit in c.block_bits[1:]} == set(range(8))
    for magic, word in (("block", B.BLOCK_MAGIC), ("end-of-stream", B.END_MAGIC)):
        seen = set()
        for c in cases:
            if c.name.startswith(magic + "-magic-in-the-data"):
                real = [bit - 80 for bit in c.block_bits] if magic == "block" else [c.consumed * 8 - 80 - k for k in range(8)]
                inside = [at for at in occurrences(bits_of(c.stream), word) if at not in real]
                assert len(inside) == 1 and inside[0] > c.block_bits[0], c.name
                seen.add(inside[0] % 8)
        assert seen == set(range(8)), magic


@pytest.mark.parametrize("seed", range(3))
def test_random_streams_mean_what_they_were_built_for(seed):
    rnd = random.Random(0xB21B + seed)
    constructs = set()
    for i in range(40):
        strict = i % 2 == 0
        c = B.random_stream(rnd, strict, constructs=None if strict else constructs, big=i % 16 == 1)
        assert O.bzip2(c.stream) == (0, c.plain, c.consumed), (seed, i)
        if strict:
            assert c.libbz2_ok and libbz2_agrees(c), (seed, i)
    # the random set must not shrink to what libbz2 would have read
    for construct in ("multi-cycle L", "surplus selectors", "over-subscribed table", "wrapped run", "block size over the level"):
        assert construct in constructs, construct
