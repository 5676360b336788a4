"""GPU tier: the BZip2 streams built symbol by symbol (tests/_bzip2_build.py) through the C ABI on the MI355X -- the assembly symbol
loop and its C++ twin, the inverse BWT inside the block's wavefront and as the team kernels, the host framing with its magic
candidates, the relaunch of a block whose column outgrows its workspace -- against what the builder's model and the oracle (reference
Sources/BZip2) say.  tests/test_bzip2_build.py holds the builder to the oracle first."""
import random

import pytest

import _bzip2_build as B
import _oracle as O
import _soak as K
import swcompression_amd as swc
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu

RELAUNCH = ("BZh1-with-L-of-", "one-run-of-2^1", "one-run-of-2^20", "one-run-of-2^23")


@pytest.fixture(params=[(0, 0), (2, 0), (0, 1), (2, 1)], ids=["fused-isa", "team-isa", "fused-cxx", "team-cxx"])
def engine(request):
    """Stage 3a inside the block's wavefront / as kernels of its own whatever the launch (tuning "bzip2_team_walk" 0 / 2), the symbol
    loop in assembly / as its C++ twin ("bzip2_hot_cxx" 0 / 1); both set and restored as test_gpu_bzip2.py does."""
    from swcompression_amd import _lib
    lib = _lib.load()
    walk, cxx = request.param
    assert lib.swc_set_tuning(b"bzip2_team_walk", walk) == 0 and lib.swc_set_tuning(b"bzip2_hot_cxx", cxx) == 0
    yield request.param
    lib.swc_set_tuning(b"bzip2_team_walk", 1)
    lib.swc_set_tuning(b"bzip2_hot_cxx", 0)


@pytest.fixture
def output_cap():
    O.lib.refcpu_set_max_output(B.MAX_OUTPUT)
    yield
    O.lib.refcpu_set_max_output(1 << 30)


def _decompress(data):
    try:
        return 0, swc.BZip2.decompress(data)
    except swc.SWCError as e:
        return e.status, e.data


@pytest.mark.parametrize("long_columns", [False, True], ids=["to-70000", "longer"])
def test_every_good_stream_in_one_launch(engine, long_columns):
    """The status-0 cases as ONE unarchive_many -- those whose columns stay within 70,000 bytes, and (a launch of its own, to keep
    each test short) the longer ones: the runs of 17 .. 22 digits, launched again with a larger workspace.  Bytes equal the model's.
    Once per parametrisation each, and so not here: the run of 2^23 and the other relaunch cases (test_columns_that_outgrow_their_
    workspace), the 2.59 MB RLE1 block (test_single_blocks_as_one_batch_at_exact_capacities)."""
    cases = [c for c in B.directed_cases() if c.status == 0 and not c.name.startswith(RELAUNCH) and c.name != "rle1-50000-of-aaaa-ff"
             and (max(c.l_len) > 70000) == long_columns]
    assert len(cases) >= (10 if long_columns else 300)
    got = swc.unarchive_many("bzip2", [c.stream for c in cases])
    for c, g in zip(cases, got):
        assert g[0] == 0, "%s: status %d" % (c.name, g[0])
        assert g[1] == c.plain, "%s: bytes differ (%d, expected %d)" % (c.name, len(g[1]), len(c.plain))


def test_every_error_case_one_by_one(engine, output_cap):
    """Status as the oracle's; wrongCRC carries the oracle's bytes (the rule of test_gpu_bzip2.py::_same)."""
    cases = [c for c in B.directed_cases() if c.status != 0]
    assert len(cases) >= 25
    for c in cases:
        st, out, _ = O.bzip2(c.stream)
        assert st == c.status, c.name
        got = _decompress(c.stream)
        assert got[0] == st, "%s: status %d, oracle %d" % (c.name, got[0], st)
        if st == 210:
            assert got[1] == out, c.name


def test_built_streams_back_to_back(engine):
    for name, data in B.multi_cases():
        st, outs = O.bzip2_multi(data)[:2]
        assert st == 0 and swc.BZip2.multi_decompress(data) == outs, name
        assert swc.BZip2.decompress(data) == outs[0], name


def test_single_blocks_as_one_batch_at_exact_capacities(engine):
    """Every single-block status-0 case that is not empty and needs no relaunch as ONE DeviceBatch("bzip2_block"): `extra` the bit
    offset of the block body, `dict_values` the stored CRC, the capacity exactly the output's length -- the 2.59 MB RLE1 block among
    them.  Left out: an empty block (no output to give a capacity for, nothing to compare), and columns over 70,000 bytes -- the batch
    cuts one workspace for the whole launch and never enlarges it (904 is its answer); those go through BZip2.decompress above."""
    cases = [c for c in B.directed_cases() if c.status == 0 and len(c.block_bits) == 1 and len(c.plain) > 0 and c.l_len[0] <= 70000]
    assert len(cases) >= 200
    b = DeviceBatch("bzip2_block", [c.stream for c in cases], [len(c.plain) for c in cases], extra=[c.block_bits[0] for c in cases],
                    dict_values=[c.block_crc[0] for c in cases])
    b.launch(sync=True)
    r = b.results()
    for i, c in enumerate(cases):
        assert int(r["status"][i]) == 0 and int(r["out_len"][i]) == len(c.plain), (c.name, int(r["status"][i]), int(r["out_len"][i]))
        assert b.output(i, len(c.plain)) == c.plain, c.name


def test_columns_that_outgrow_their_workspace(engine):
    """A BZh1 stream whose block is longer than the level allows, a stream of under 100 bytes with one long run: run_units launches
    the block again with four times the capacity until it fits -- status 0 and the model's bytes, never 904."""
    cases = [c for c in B.directed_cases() if c.name.startswith(RELAUNCH)]
    assert len(cases) == 7
    for c in cases:
        got = _decompress(c.stream)
        assert got[0] == 0, "%s: status %d" % (c.name, got[0])
        assert got[1] == c.plain, c.name


SOAK_SEEDS = (0, 1, 2)       # picked on the CPU: the oracle answers 901 on none of their damaged streams (the limit below: 5 %)


@pytest.mark.parametrize("seed", SOAK_SEEDS)
def test_random_built_streams_clean_and_damaged(seed, output_cap):
    """64 random built streams per seed, clean ones in ONE unarchive_many (team kernels, then the block's own wavefront), damaged
    copies one by one under the _same rule.  A damaged stream on which the oracle says 901 (its output cap) is left out: at most 5 %
    of them may be."""
    from swcompression_amd import _lib
    lib = _lib.load()
    rnd = random.Random(0xB25 + 977 * seed)
    cases = [B.random_stream(rnd, i % 2 == 0, name="random-%d-%d" % (seed, i), big=i % 16 == 1) for i in range(64)]
    damaged = [K.damage(rnd, cases[rnd.randrange(len(cases))].stream) for _ in range(64)]
    exp = [O.bzip2(z) for z in damaged]
    keep = [i for i, e in enumerate(exp) if e[0] != 901]
    assert len(damaged) - len(keep) <= len(damaged) * 5 // 100
    try:
        for mode in (2, 0):
            assert lib.swc_set_tuning(b"bzip2_team_walk", mode) == 0
            got = swc.unarchive_many("bzip2", [c.stream for c in cases])
            for c, g in zip(cases, got):
                assert g[0] == 0 and g[1] == c.plain, "%s, team walk %d: status %d" % (c.name, mode, g[0])
            for i in keep:
                got1 = _decompress(damaged[i])
                assert got1[0] == exp[i][0], "seed %d, team walk %d, damaged %d: status %d, oracle %d" % (seed, mode, i, got1[0], exp[i][0])
                if exp[i][0] in (0, 210):
                    assert got1[1] == exp[i][1], "seed %d, team walk %d, damaged %d: bytes differ" % (seed, mode, i)
    finally:
        lib.swc_set_tuning(b"bzip2_team_walk", 1)
