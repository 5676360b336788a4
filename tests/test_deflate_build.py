"""CPU tier: the self-check of the Deflate stream builder (tests/_deflate_build.py).  Before any built stream is compared with
the kernels, the oracle must return exactly what the builder meant -- (0, plain, body length), or the status an error case was
built for -- and zlib must agree wherever it can: on every stream whose code sets are ones it accepts.  Streams with incomplete or
over-subscribed sets are checked against the oracle only (zlib refuses them by design; the reference validates neither)."""
import random
import zlib

import pytest

import _deflate_build as B
import _oracle as O


def _zlib_agrees(stream, plain, body_len):
    d = zlib.decompressobj(-15)
    return d.decompress(stream) == plain and d.eof and d.unused_data == stream[body_len:]


def test_bit_writer_against_the_bit_list_writer():
    import _streams as S
    rnd = random.Random(1)
    a, b = B.BitWriter(), S.LsbBitWriter()
    for _ in range(5000):
        n = rnd.randrange(0, 17)
        v = rnd.getrandbits(n) if n else 0
        if rnd.randrange(2):
            a.bits(v, n), b.write(v, n)
        else:
            a.code(v, n), b.code(v, n)
        if rnd.randrange(200) == 0:
            assert a.bit_length() == len(b.bits)
    assert a.data() == b.data()


@pytest.mark.parametrize("maxbits,deep", [(15, 0.0), (15, 0.5), (15, 1.0), (7, 0.9), (9, 0.3)])
def test_random_complete_lengths_are_complete(maxbits, deep):
    rnd = random.Random(maxbits * 10 + int(deep * 7))
    for n in (2, 3, 19, 30, 128, 286):
        if n > 1 << maxbits:
            continue
        for _ in range(20):
            got = B.random_complete_lengths(rnd, range(n), maxbits, deep)
            assert sorted(got) == list(range(n)) and max(got.values()) <= maxbits and B.is_complete(got.values())
    assert max(B.random_complete_lengths(rnd, range(286), 15, 1.0).values()) == 15


def test_header_runs_cross_the_boundary_and_spell_the_lengths():
    rnd = random.Random(5)
    for policy in ("none", "greedy", "random"):
        for _ in range(50):
            lengths = [rnd.choice([0, 0, 0, 5, 5, 7, rnd.randrange(16)]) for _ in range(rnd.randrange(258, 319))]
            spelled, prev = [], None
            for sym, extra, first, count in B.header_symbols(lengths, policy, rnd):
                assert first == len(spelled)
                if sym == 16:
                    assert 3 <= count <= 6 and count == extra + 3 and prev not in (None, 0)
                    spelled += [prev] * count
                elif sym >= 17:
                    assert count == extra + (3 if sym == 17 else 11) and count <= (10 if sym == 17 else 138)
                    spelled += [0] * count
                    prev = 0
                else:
                    spelled.append(sym)
                    prev = sym
                prev = spelled[-1]
            assert spelled == lengths
            assert policy != "none" or all(s[0] < 16 for s in B.header_symbols(lengths, policy, rnd))


def test_directed_streams_mean_what_they_were_built_for():
    cases = B.directed_cases()
    assert len(cases) >= 60 and [(c.name, c.stream, c.plain) for c in cases] == B.directed_streams()
    for c in cases:
        st, out, cons = O.deflate(c.stream)
        if c.status == 0:
            assert (st, out, cons) == (0, c.plain, c.body_len), c.name
            if c.zlib_ok:
                assert _zlib_agrees(c.stream, c.plain, c.body_len), c.name
            else:
                with pytest.raises(zlib.error):
                    zlib.decompressobj(-15).decompress(c.stream)
        else:
            assert c.plain is None and st == c.status, "%s: oracle status %d" % (c.name, st)
    by_name = {c.name: c for c in cases}
    assert by_name["error-distance-beyond-output-behind-5000"].status == 900 and by_name["error-fixed-literal-286-behind-70000"].status == 103
    assert by_name["symbol-16-first"].status == 103 and by_name["no-distance-code-and-a-length-symbol"].status == 104
    assert len(by_name["stored-blocks-of-65535-bytes"].plain) > 2 * 65535


@pytest.mark.parametrize("seed", range(3))
def test_random_streams_mean_what_they_were_built_for(seed):
    rnd = random.Random(0xB111D + seed)
    styles = set()
    for i in range(20):
        style = i % 4
        z, p, body = B.random_stream(rnd, rnd.choice([0, 1, 9, 300, 4000, 65536, 70000, 200000]), style)
        assert O.deflate(z) == (0, p, body), (seed, i)
        assert _zlib_agrees(z, p, body), (seed, i)
        styles.add(style)
    assert styles == {0, 1, 2, 3}
