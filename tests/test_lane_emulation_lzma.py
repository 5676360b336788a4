"""CPU tier: the LZMA / LZMA2 wave decoder (swcompression_amd/csrc/lzma_wave.h) built for the host as a
single logical lane vs the oracle (reference Sources/LZMA/*.swift, Sources/LZMA2/*.swift)."""
import functools
import lzma as _pylzma

import numpy as np
import pytest

import _emu as E
import _lzma_build as B
import _oracle as O
import _streams as S


@pytest.fixture(autouse=True, params=[0, 1], ids=["coders-in-lds", "coder-cache"])
def _model_mode(request):
    """Every test runs in both model layouts of the device kernels (lzma_wave.h: all literal coders in LDS / LDS as a cache of
    four coders with the workspace behind it)."""
    E.LZMA_MODE = request.param
    yield
    E.LZMA_MODE = 0


def test_lzma2_valid():
    cases = S.lzma2_valid()
    res = E.lzma2([z for z, _, _ in cases], [max(len(x), 1) for _, _, x in cases], [db for _, db, _ in cases])
    for r, (z, db, x) in zip(res, cases):
        assert r[:3] == (0, x, len(z))
        assert O.lzma2(z, db) == (0, x, len(z))


def test_lzma2_fuzz():
    O.lib.refcpu_set_max_output(1 << 24)
    cases = S.lzma2_fuzz()
    exp = [O.lzma2(z, db) for z, db in cases]
    res = E.lzma2([z for z, _ in cases], [max(len(e[1]), 1) + 64 for e in exp], [db for _, db in cases])
    for r, e, (z, db) in zip(res, exp, cases):
        if e[0] == 901:
            continue
        assert r[0] == e[0], (z[:16].hex(), db)
        if e[0] == 0:
            assert r[1] == e[1] and r[2] == e[2]
    O.lib.refcpu_set_max_output(1 << 30)


def test_lzma_alone_valid_and_raw_fuzz():
    O.lib.refcpu_set_max_output(1 << 24)
    ins, props, dss, szs, exp = [], [], [], [], []
    for z, x in S.lzma_alone_valid():
        b = z[0]
        p = (b % 9, (b // 9) % 5, (b // 9) // 5)
        ds = int.from_bytes(z[1:5], "little")
        for size in (-1, len(x)):
            ins.append(z[13:]); props.append(p); dss.append(ds); szs.append(size)
            exp.append(O.lzma_raw(z[13:], p[0], p[1], p[2], ds, size))
            if size == -1 and p[2] < 4:
                assert exp[-1][:2] == (0, x)
            # pb == 4: a VALID stream can reach state 11 / posState 15, where the reference indexes
            # probabilities[432] (LZMADecoder.swift:186-187) and traps
    for body, p, ds, size in S.lzma_raw_fuzz():
        ins.append(body); props.append(p); dss.append(ds); szs.append(size)
        exp.append(O.lzma_raw(body, p[0], p[1], p[2], ds, size))
    res = E.lzma(ins, [max(len(e[1]), 1) + 300 for e in exp], props, dss, szs)
    for i, (r, e) in enumerate(zip(res, exp)):
        if e[0] == 901:
            continue
        assert r[0] == e[0], (i, props[i], dss[i], szs[i], ins[i][:16].hex())
        if e[0] == 0:
            assert r[1] == e[1] and r[2] == e[2]
    O.lib.refcpu_set_max_output(1 << 30)


def test_capacity_is_reported():
    cases = S.lzma2_valid(sizes=(5000, 70000))[:6]
    res = E.lzma2([z for z, _, _ in cases], [len(x) // 2 for _, _, x in cases], [db for _, db, _ in cases])
    assert all(r[0] == 901 for r in res)


def test_every_literal_coder_in_turn():
    """The coder cache under pressure: a payload whose previous-byte classes cycle through all coders of every model shape the
    system encoder produces (lc + lp <= 4: up to sixteen coders for four slots), so that slots are written back and come back
    with their adapted cells.  (Larger models -- legal in .lzma, never written by liblzma -- are reached by the raw fuzz above.)"""
    rng = np.random.Generator(np.random.PCG64(0x5C0DE + 401))
    n = 60000
    base = (np.arange(n) * 37 % 256).astype(np.uint8)
    noise = rng.integers(0, 256, n, dtype=np.uint8)
    x = np.where(rng.random(n) < 0.7, base, noise).astype(np.uint8).tobytes()
    ins, props, dss, szs, exp = [], [], [], [], []
    for lc, lp, pb in ((3, 0, 2), (4, 0, 0), (0, 4, 2), (2, 2, 0), (0, 0, 0), (1, 3, 4)):
        f = [{"id": _pylzma.FILTER_LZMA1, "lc": lc, "lp": lp, "pb": pb, "dict_size": 1 << 16}]
        z = _pylzma.compress(x, format=_pylzma.FORMAT_RAW, filters=f)
        ins.append(z); props.append((lc, lp, pb)); dss.append(1 << 16); szs.append(len(x))
        exp.append(O.lzma_raw(z, lc, lp, pb, 1 << 16, len(x)))
        assert exp[-1][:2] == (0, x)
    res = E.lzma(ins, [len(x) + 16] * len(ins), props, dss, szs)
    for r, e, p in zip(res, exp, props):
        assert r[0] == e[0] and r[1] == e[1] and r[2] == e[2], p


def test_random_payload_mixtures_every_model_shape():
    """Seeded random mixtures of text-like, binary, repetitive and random pieces under every (lc, lp, pb) with lc + lp <= 4, as
    LZMA1 and as LZMA2 with small chunks (several model resets per stream): both model layouts against the oracle."""
    import random
    rnd = random.Random(0x5C0DE + 402)
    rng = np.random.Generator(np.random.PCG64(0x5C0DE + 403))

    def piece(kind, n):
        if kind == 0:
            return bytes(rnd.choice(b"etaoin shrdlu,.\nETAOIN0123") for _ in range(n))
        if kind == 1:
            return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        if kind == 2:
            return (bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 9))) * (n // 2 + 1))[:n]
        return (np.cumsum(rng.integers(-3, 4, n)) & 0xFF).astype(np.uint8).tobytes()

    shapes = [(lc, lp, pb) for lc in range(5) for lp in range(5 - lc) for pb in (0, 2, 4)]
    ins1, props, dss, szs, want1 = [], [], [], [], []
    ins2, want2 = [], []
    for k, (lc, lp, pb) in enumerate(shapes):
        x = b"".join(piece(rnd.randrange(4), rnd.randrange(1, 3000)) for _ in range(rnd.randrange(1, 12)))
        f1 = [{"id": _pylzma.FILTER_LZMA1, "lc": lc, "lp": lp, "pb": pb, "dict_size": 1 << 16}]
        z1 = _pylzma.compress(x, format=_pylzma.FORMAT_RAW, filters=f1)
        ins1.append(z1); props.append((lc, lp, pb)); dss.append(1 << 16); szs.append(len(x) if k & 1 else -1); want1.append(x)
        f2 = [{"id": _pylzma.FILTER_LZMA2, "lc": lc, "lp": lp, "pb": pb, "dict_size": 1 << 16}]
        ins2.append(_pylzma.compress(x, format=_pylzma.FORMAT_RAW, filters=f2)); want2.append(x)
    res = E.lzma(ins1, [len(x) + 300 for x in want1], props, dss, szs)
    for r, z, x, p, ds, sz in zip(res, ins1, want1, props, dss, szs):
        e = O.lzma_raw(z, p[0], p[1], p[2], ds, sz)
        if e[0] == 901:
            continue
        assert r[0] == e[0] and (e[0] != 0 or (r[1] == e[1] and r[2] == e[2])), p
    db = 16   # 64 KiB dictionary
    res = E.lzma2(ins2, [max(len(x), 1) for x in want2], [db] * len(ins2))
    for r, z, x, p in zip(res, ins2, want2, shapes):
        e = O.lzma2(z, db)
        assert r[0] == e[0], p       # (pb = 4: a valid stream can reach the index the reference traps on)
        if e[0] == 0:
            assert r[:3] == (0, x, len(z)) and e[1] == x, p


# ------------------------------------------------------------------------ streams built decision by decision (tests/_lzma_build.py)
@functools.lru_cache(maxsize=None)
def _directed_expectations():
    """The oracle on the directed set of _lzma_build.py, computed once; each case held to the KIND of result it was built for (a
    builder that drifted would otherwise turn the comparison into oracle == kernel on the wrong streams)."""
    cases = B.directed_cases()
    exp = [O.lzma2(c.stream, c.dict_byte) if c.kind == "lzma2" else O.lzma_raw(c.stream, *c.props) for c in cases]
    for c, e in zip(cases, exp):
        assert e == (0, c.plain, c.consumed) if c.status == 0 else e[0] == c.status, c.name
    return cases, exp


def _emulate(cases, caps):
    """Built cases of both kinds through the emulated kernel, in the order given."""
    res = [None] * len(cases)
    i2 = [i for i, c in enumerate(cases) if c.kind == "lzma2"]
    i1 = [i for i, c in enumerate(cases) if c.kind == "lzma"]
    for i, r in zip(i2, E.lzma2([cases[i].stream for i in i2], [caps[i] for i in i2], [cases[i].dict_byte for i in i2])):
        res[i] = r
    for i, r in zip(i1, E.lzma([cases[i].stream for i in i1], [caps[i] for i in i1], [cases[i].props[:3] for i in i1],
                               [cases[i].props[3] for i in i1], [cases[i].props[4] for i in i1])):
        res[i] = r
    return res


def _check_built(cases, exp, res, label=""):
    for c, e, r in zip(cases, exp, res):
        assert r[0] == e[0], "%s%s: status %d, oracle %d" % (label, c.name, r[0], e[0])
        if e[0] == 0:
            assert r[3] == len(e[1]) and r[2] == e[2], "%s%s: %d bytes out, %d consumed; oracle %d, %d" % (label, c.name, r[3], r[2], len(e[1]), e[2])
            assert r[1] == e[1], "%s%s: bytes differ" % (label, c.name)


def test_built_streams_directed():
    """What liblzma never writes (tests/_lzma_build.py: directed_cases): property changes and dictionary resets in mid-stream, 0x80
    behind a stored chunk, lc + lp up to 12, every packet kind from every state, every length through both coders, every pos slot
    up to 2 MiB, end markers inside chunks, dictionaries of 0 .. 3 bytes.  Valid streams at EXACT capacity."""
    cases, exp = _directed_expectations()
    _check_built(cases, exp, _emulate(cases, [max(len(e[1]), 1) if e[0] == 0 else len(e[1]) + 300 for e in exp]))


def test_built_streams_one_byte_short_of_capacity():
    cases, exp = _directed_expectations()
    pick = [i for i, c in enumerate(cases) if c.status == 0 and len(c.plain) > 1 and
            c.name.split("-")[0] in ("states", "copy", "every", "probabilities", "0x80", "4KiB", "raw", "properties", "end")]
    assert len(pick) >= 30
    res = _emulate([cases[i] for i in pick], [len(cases[i].plain) - 1 for i in pick])
    for i, r in zip(pick, res):
        assert r[0] == 901, "%s: status %d" % (cases[i].name, r[0])


@pytest.mark.parametrize("seed", range(2))
def test_built_streams_random(seed):
    """Seeded random built streams, half of them restricted to what liblzma decodes, the other half drawn from everything the
    reference accepts."""
    import random
    rnd = random.Random(0x12A4B00 + seed)
    cases = [B.random_stream(rnd, rnd.choice([1, 9, 300, 4000, 20000]), i % 2 == 0) for i in range(100)]
    exp = [O.lzma2(c.stream, c.dict_byte) if c.kind == "lzma2" else O.lzma_raw(c.stream, *c.props) for c in cases]
    for i, (c, e) in enumerate(zip(cases, exp)):
        assert e == (0, c.plain, c.consumed), "the builder and the oracle disagree on a stream it built (seed %d, stream %d)" % (seed, i)
    _check_built(cases, exp, _emulate(cases, [max(len(c.plain), 1) for c in cases]), "seed %d, " % seed)
