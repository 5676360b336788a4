"""The follow-up literal of the provisional decode (csrc/inflate_sync.h, decode_chunk_prov) on the host emulation: phase 1 byte for
byte, and both phases, against the same sources built with -DSWC_SYNC_NO_FOLLOW=1 (one code per step) and against the oracle; the
form that takes the follow-up's bits from the held window (-DSWC_SYNC_FOLLOW_HELD=1) is held to the same.  The directed streams
are checked to contain what they were built for by a model of the steps (_deflate_follow_cases.steps), and the model is checked
against the steps the emulated decoder counts."""
import random
import zlib

import pytest

import _deflate_follow_cases as FC
import _emu_deflate_phase1 as F
import _oracle as O
from swcompression_amd import corpus


@pytest.fixture(params=[0, 1, 2], ids=["forward", "reverse", "shuffled"])
def order(request):
    F.set_order(request.param)
    yield request.param
    F.set_order(0)


@pytest.fixture(params=[0, 1], ids=["one-wave", "team"])
def team(request):
    F.set_team(request.param)
    yield request.param
    F.set_team(0)


CASES = FC.directed()
EXPECTED = {c[0]: O.deflate(c[1]) for c in CASES}
_STEPS = {c[0]: FC.steps(c[3], c[4]) for c in CASES}
_STEPS_HELD = {c[0]: FC.steps(c[3], c[4], held=True) for c in CASES}


def _cap(c):
    return c[2] if c[2] is not None else max(len(EXPECTED[c[0]][1]), 1)


def test_the_streams_hold_what_they_were_built_for():
    st = _STEPS
    # every count of literals % 4 at the start of a step, behind a literal, a pair and a distance; never behind a length
    for r in range(4):
        for kind, own in (("literal", "lit"), ("pair", "pair"), ("distance", "dist")):
            assert any(k == 0 and nl == r and o == own and take for k, nl, o, take, _ in st["count-%d-literal-behind-a-%s" % (r, kind)]), (r, kind)
        assert any(nl == r and o == "len" for _, nl, o, _, _ in st["count-%d-literal-behind-a-length" % r])
    assert not any(take for v in st.values() for _, _, o, take, _ in v if o in ("len", "eob", "bad"))
    # a group completed by the step's literal with a follow-up behind it, and by the follow-up
    done = {(d, take) for n, v in st.items() if n.startswith("group-") for _, _, _, take, d in v}
    assert {(1, True), (2, True), (1, False)} <= done
    assert any(d == 1 and take for _, _, _, take, d in st["group-first-literal-completes"])
    # the literal at the end of a sub-chunk: taken one bit in front of it, not taken at it (the neighbour's first step is that literal)
    for k in (1, 2, 63):
        for front, own in (("literal", "lit"), ("pair", "pair")):
            last = {d: [s for s in st["literal-at-boundary-%d%+d-behind-a-%s" % (k, d, front)] if s[0] == k - 1][-1] for d in (0, -1, 1)}
            assert last[0][2:4] == (own, False) and last[-1][2:4] == (own, True) and last[1][2:4] == (own, False), (k, front, last)
            first = [s for s in st["literal-at-boundary-%d+0-behind-a-%s" % (k, front)] if s[0] == k][0]
            assert first[2] == "lit" and first[1] == 0
    # candidates that are not taken, and those that are
    for name, own in (("end-of-block", "eob"), ("length", "len"), ("pair", "pair"), ("link-11-bits", "long"), ("link-12-bits", "long"), ("symbol-286", "bad"), ("symbol-287", "bad")):
        v = st["candidate-" + name]
        assert any(v[i][2] != "len" and not v[i][3] and v[i + 1][2] == own for i in range(len(v) - 1)), name   # a step that could have, and did not
    assert sum(take for _, _, o, take, _ in st["candidate-code-of-10-bits"]) > sum(take for _, _, o, take, _ in st["candidate-link-11-bits"])
    # form (b): with the largest pair in front, the follow-up fits the held window at some offsets of the dword and not at others
    big = lambda steps, off: [s for s in steps["largest-pair-at-bit-%d-of-its-dword" % off] if s[2] == "pair"][-1][3]   # (the last pair of the stream)
    fits = [big(_STEPS_HELD, off) for off in range(32)]
    assert fits == [off + 23 <= FC.HELD_MAX for off in range(32)] and True in fits and False in fits
    assert all(big(st, off) for off in range(32))
    # the literal that ends beyond the input is once a step of its own and once a follow-up
    ends = [st["literal-ends-beyond-the-input-%d" % k][-1] for k in (0, 1)]
    assert sorted(e[3] for e in ends) == [False, True], ends
    assert all(EXPECTED["literal-ends-beyond-the-input-%d" % k][0] != 0 for k in (0, 1))
    assert EXPECTED["distance-exactly-the-output"][0] == 0 and EXPECTED["distance-one-beyond-the-output"][0] != 0
    assert EXPECTED["candidate-symbol-286"][0] != 0 and EXPECTED["candidate-symbol-287"][0] != 0
    assert all(e[0] == 0 for n, e in EXPECTED.items() if not n.startswith(("literal-ends-beyond", "distance-one-beyond", "candidate-symbol-28")))


def test_the_emulated_decoder_takes_the_follow_ups_of_the_model():
    """One wave, lanes forward: the provisional pass of each build takes as many steps fewer than the build with one code per step as
    the model has follow-ups (whatever else counts as a step -- the general passes of a round that fell back -- is the same in all
    three builds)."""
    for c in CASES:
        name = c[0]
        if name.startswith("pending-literals"):
            continue                                    # (two blocks: the model covers the second)
        base = F.counted(F.single, c[1], _cap(c))[4]
        for lib, model in ((F.shipped, _STEPS[name]), (F.held, _STEPS_HELD[name])):
            assert base - F.counted(lib, c[1], _cap(c))[4] == sum(s[3] for s in model), name


def test_directed_streams_phase_1_is_the_one_with_one_code_per_step(order, team):
    for c in CASES:
        for aux in (0, 1 | 4):          # alone; SWC_DEFLATE_JOINED | SWC_DEFLATE_LINKED: distances may reach into a history
            want = F.phase1(F.single, c[1], _cap(c), aux, team)
            assert F.phase1(F.shipped, c[1], _cap(c), aux, team) == want, (c[0], aux)
            assert F.phase1(F.held, c[1], _cap(c), aux, team) == want, (c[0], aux, "held window")


def test_directed_streams_against_the_oracle(order, team):
    zs, caps = [c[1] for c in CASES], [_cap(c) for c in CASES]
    ref = F.inflate(F.single, zs, caps)
    for lib in (F.shipped, F.held):
        res = F.inflate(lib, zs, caps)
        for c, r, q in zip(CASES, res, ref):
            st, out, cons = EXPECTED[c[0]]
            assert r == q, c[0]
            assert r[0] == st, (c[0], r[0], st)
            if st == 0:
                assert (r[1], r[2], r[3]) == (out, cons, len(out)), c[0]


def test_capacity_inside_a_follow_up_run(team):
    c = next(c for c in CASES if c[0] == "group-nine")
    out = EXPECTED[c[0]][1]
    for cap in (len(out) - 1, len(out) - 4, 301, 302):
        got = F.inflate(F.shipped, [c[1]], [cap])
        assert got == F.inflate(F.single, [c[1]], [cap]) and got[0][1] == out[:cap]


def _all_literal(n, seed):
    rnd = random.Random(seed)
    return bytes(rnd.choice(b"etaoinshrdlu ,.") for _ in range(n))


MEMBERS = [("text", corpus.p_text(65536, 11)), ("mix", corpus.p_mix(65536, 12)), ("all-literal", _all_literal(65536, 13))]


@pytest.mark.parametrize("kind", [m[0] for m in MEMBERS])
def test_members_of_64k_against_zlib(kind, order, team):
    plain = dict(MEMBERS)[kind]
    if kind == "all-literal":
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        z = c.compress(plain) + c.flush()
    else:
        z = corpus.deflate_raw(plain, 6)
    assert zlib.decompress(z, -15) == plain
    want = F.phase1(F.single, z, len(plain), 0, team)
    assert want[:3] == (0, len(plain), len(z))
    assert F.phase1(F.shipped, z, len(plain), 0, team) == want
    assert F.phase1(F.held, z, len(plain), 0, team) == want
    assert F.inflate(F.shipped, [z], [len(plain)]) == [(0, plain, len(z), len(plain))]


def test_small_streams_phase_1(order, team):
    for k, z in enumerate(FC.small_streams(random.Random(2600))):
        st, out, cons = O.deflate(z)
        assert st == 0
        want = F.phase1(F.single, z, len(out), 0, team)
        assert F.phase1(F.shipped, z, len(out), 0, team) == want and F.phase1(F.held, z, len(out), 0, team) == want, k
        assert want[:3] == (0, len(out), cons)
