"""GPU tier of the PAIR entries of the direct lit/len table (csrc/inflate_sync.h): the directed streams of _deflate_pairs_cases in one
launch on the MI355X -- one wave per stream, a team per stream, the team forced; the workgroup resolver and the wave copier --
and 2,600 small streams so that the wave copier and the ordering kernels run; outputs against the oracle, the CRC-32 the launch
leaves (swc_batch_decompress_crc32_ws) against zlib's."""
import random
import zlib

import numpy as np
import pytest

import _deflate_build as B
import _deflate_linked_cases as L
import _deflate_pairs_cases as PC
import _oracle as O
from swcompression_amd import _lib
from swcompression_amd.batch import DeviceBatch
from test_gpu_deflate_linked import check_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def directed():
    """[(name, stream, capacity, (status, bytes, in_consumed) of the oracle)], computed once"""
    out = []
    for name, z, cap in PC.directed():
        e = O.deflate(z)
        out.append((name, z, cap if cap is not None else max(len(e[1]), 1), e))
    assert len(out) <= 512 and {e[0] for _, _, _, e in out} == {0, PC.E_TRAP, PC.E_NOT_FOUND}
    return out


@pytest.fixture(scope="module")
def linked():
    return [(name, run, L.expect(run)) for name, run in PC.linked_runs().items()]


def _knobs(lib, team, copier):
    assert lib.swc_set_tuning(b"lz_copier", copier) == 0 and lib.swc_set_tuning(b"deflate_team", team) == 0


def _reset(lib):
    lib.swc_set_tuning(b"lz_copier", 1)
    lib.swc_set_tuning(b"deflate_team", 1)


@pytest.mark.parametrize("copier", [1, -1])
@pytest.mark.parametrize("team", [0, 1, -1])
def test_directed_streams_in_one_launch(directed, linked, team, copier):
    lib = _lib.load()
    units = [u for _, run, _ in linked for u in run]
    n_linked = len(units)
    _knobs(lib, team, copier)
    try:
        b = DeviceBatch("deflate", [u["data"] for u in units] + [z for _, z, _, _ in directed], [u["cap"] for u in units] + [cap for _, _, cap, _ in directed],
                        aux=[u["aux"] for u in units] + [0] * len(directed), guard=16)
        b.crc32_async()          # (allocates the CRC buffer: the launch below leaves the CRCs in it)
        b.launch(sync=True)
        assert b._crc_current and b.n <= 512
        crcs = b._crc_buf.cpu().numpy().view(np.uint32)
        check_batch(b, linked, crcs)
        assert [exp[1][0] for _, _, exp in linked] == [0, PC.E_TRAP]
        r = b.results()
        for k, (name, z, cap, (st, out, cons)) in enumerate(directed):
            i = n_linked + k
            if cap < len(out):
                assert int(r["status"][i]) == PC.E_CAPACITY and int(r["out_len"][i]) == len(out) and b.output(i, cap) == out[:cap], name
                assert int(crcs[i]) == zlib.crc32(out[:cap]), name + ": CRC-32"
                continue
            assert int(r["status"][i]) == st, name
            if st == 0:
                assert (int(r["out_len"][i]), int(r["in_consumed"][i])) == (len(out), cons), name
                assert b.output(i, len(out)) == out, name
                assert int(crcs[i]) == zlib.crc32(out), name + ": CRC-32"
        assert b.unwritten_intact()
    finally:
        _reset(lib)


@pytest.mark.parametrize("copier", [1, -1])
@pytest.mark.parametrize("team", [0, 1, -1])
def test_2600_small_streams(team, copier):
    """2,600 streams of 2 .. 8 KiB, sixteen distinct ones: built token by token over the pairing code sets, and zlib's."""
    lib = _lib.load()
    rnd = random.Random(2600)
    distinct = []
    for c in range(16):
        n = rnd.randrange(2048, 8193)
        if c % 2:
            plain = PC.TEXT[c * 100:c * 100 + n]
            comp = zlib.compressobj(6, zlib.DEFLATED, -15)
            z = comp.compress(plain) + comp.flush()
        else:
            s = PC.Stream(prefix=200 + c)
            s.header()
            while s.n_out < n - 40:
                s.put(*[rnd.choice([97, 98, 120, 121]) for _ in range(rnd.randrange(1, 30))], rnd.choice([PC.PAIR, PC.MATCH, ("sym", 265, 1, 1, 0), ("sym", 273, 5, 2, 0)]))
            s.put(*([97] * (n - s.n_out)))
            s.eob()
            z = s.data()
        st, out, cons = O.deflate(z)
        assert st == 0 and len(out) == n
        distinct.append((z, out, cons))
    reps = 2600
    _knobs(lib, team, copier)
    try:
        b = DeviceBatch("deflate", [distinct[i % 16][0] for i in range(reps)], [len(distinct[i % 16][1]) for i in range(reps)], guard=16)
        b.crc32_async()
        b.launch(sync=True)
        assert b._crc_current
        r = b.results()
        assert (r["status"] == 0).all()
        crcs = b._crc_buf.cpu().numpy().view(np.uint32)
        for c, (z, out, cons) in enumerate(distinct):
            assert (r["out_len"][c::16] == len(out)).all() and (r["in_consumed"][c::16] == cons).all(), c
            assert (crcs[c::16] == zlib.crc32(out)).all(), c
            for i in (c, c + 16 * 80, c + 16 * 161):
                assert b.output(i, len(out)) == out, i
        assert b.unwritten_intact()
    finally:
        _reset(lib)
