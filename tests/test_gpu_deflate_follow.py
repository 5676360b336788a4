"""GPU tier of the follow-up literal of the provisional decode (csrc/inflate_sync.h, decode_chunk_prov): the directed streams of
_deflate_follow_cases in one launch on the MI355X -- one wave per stream, a team per stream, the team forced; the workgroup
resolver and the wave copier -- and 2,600 small streams (the smallest launch the wave copy kernel takes) through the same knobs;
bytes, statuses, out_len and in_consumed against the oracle."""
import random

import pytest

import _deflate_follow_cases as FC
import _oracle as O
from swcompression_amd import _lib
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def directed():
    """[(name, stream, capacity, (status, bytes, in_consumed) of the oracle)], computed once"""
    out = []
    for c in FC.directed():
        e = O.deflate(c[1])
        out.append((c[0], c[1], c[2] if c[2] is not None else max(len(e[1]), 1), e))
    assert len(out) <= 512 and 0 in {e[0] for _, _, _, e in out} and len({e[0] for _, _, _, e in out}) >= 3
    return out


@pytest.fixture(scope="module")
def small():
    out = []
    for z in FC.small_streams(random.Random(2600)):
        st, plain, cons = O.deflate(z)
        assert st == 0 and 2048 <= len(plain) <= 4096
        out.append((z, plain, cons))
    return out


def _knobs(lib, team, copier):
    assert lib.swc_set_tuning(b"lz_copier", copier) == 0 and lib.swc_set_tuning(b"deflate_team", team) == 0


def _reset(lib):
    lib.swc_set_tuning(b"lz_copier", 1)
    lib.swc_set_tuning(b"deflate_team", 1)


@pytest.mark.parametrize("copier", [1, -1])
@pytest.mark.parametrize("team", [0, 1, -1])
def test_directed_streams_in_one_launch(directed, team, copier):
    lib = _lib.load()
    _knobs(lib, team, copier)
    try:
        b = DeviceBatch("deflate", [z for _, z, _, _ in directed], [cap for _, _, cap, _ in directed], guard=16)
        b.launch(sync=True)
        r = b.results()
        for i, (name, z, cap, (st, out, cons)) in enumerate(directed):
            assert int(r["status"][i]) == st, name
            if st == 0:
                assert (int(r["out_len"][i]), int(r["in_consumed"][i])) == (len(out), cons), name
                assert b.output(i, len(out)) == out, name
        assert b.unwritten_intact()
    finally:
        _reset(lib)


@pytest.mark.parametrize("copier", [1, -1])
@pytest.mark.parametrize("team", [0, 1, -1])
def test_2600_small_streams(small, team, copier):
    lib = _lib.load()
    reps, n = 2600, len(small)
    _knobs(lib, team, copier)
    try:
        b = DeviceBatch("deflate", [small[i % n][0] for i in range(reps)], [len(small[i % n][1]) for i in range(reps)], guard=16)
        b.launch(sync=True)
        r = b.results()
        assert (r["status"] == 0).all()
        for c, (z, out, cons) in enumerate(small):
            assert (r["out_len"][c::n] == len(out)).all() and (r["in_consumed"][c::n] == cons).all(), c
            for i in (c, c + n * 80, c + n * 161):
                assert b.output(i, len(out)) == out, i
        assert b.unwritten_intact()
    finally:
        _reset(lib)
