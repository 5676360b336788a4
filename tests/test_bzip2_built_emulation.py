"""CPU tier: every block of the built BZip2 streams (tests/_bzip2_build.py) through the three device stages compiled for the host
(swcompression_amd/csrc/bzip2_block.h, bzip2_team.h), each block at its own bit offset, in the three forms of stage 3 that
test_lane_emulation_bzip2.py runs.  The stages decode ONE block: what a stream-level case is about -- block alignment, a magic
inside block data, CRC chaining, bytes behind the end-of-stream magic -- is the GPU tier's (test_gpu_bzip2_built.py); here each of
its blocks is decoded where it stands, with the whole stream as the input."""
import contextlib
import random

import pytest

import _bzip2_build as B
import _emu as E

LCAP = 300000      # the column capacity of these runs: a block whose L is longer answers 904 (the GPU tier lets run_units enlarge it)
FORMS = {"fused": None, "team": (0, 0), "team-stealing": (5, 1)}
_random = {}


@contextlib.contextmanager
def stage3(form, order=0):
    """Stage 3a inside the block's wavefront, as kernels of its own, and with one thread that starts at team 5 and draws every team's
    tickets (the fixture of test_lane_emulation_bzip2.py), with the lanes of every SIMT region in the given order."""
    E.set_bzip2_team(FORMS[form])
    E.set_order(order)
    try:
        yield
    finally:
        E.set_bzip2_team(None)
        E.set_order(0)


def blocks_of(cases):
    """(case, block index, expected status, expected bytes) of every block the builder knows the outcome of.  A block whose column is
    longer than LCAP is expected to answer 904 and nothing else."""
    out = []
    for c in cases:
        for j, st in enumerate(c.block_status):
            if st is None:
                continue
            if c.l_len[j] > LCAP:
                st = 904
            out.append((c, j, st, c.block_plain[j] if st in (0, 210) else None))      # (210: the block decodes, its stored CRC is wrong)
    return out


def run(jobs, caps):
    return E.bzip2_block([c.stream for c, _, _, _ in jobs], [c.block_bits[j] for c, j, _, _ in jobs], [c.block_crc[j] for c, j, _, _ in jobs],
                         caps, lcap=LCAP)


def check(jobs, what):
    res = run(jobs, [len(p) if p is not None else 64 for _, _, st, p in jobs])
    for (c, j, st, plain), r in zip(jobs, res):
        where = "%s, block %d (%s)" % (c.name, j, what)
        assert r[0] == st, "status %d, expected %d: %s" % (r[0], st, where)
        if st in (0, 210):          # (210: the stored CRC is wrong, the decoded bytes are there all the same)
            assert r[3] == len(plain) and r[1] == plain, "bytes differ: " + where


@pytest.mark.parametrize("form,order", [("fused", 0), ("fused", 1), ("fused", 2), ("team", 0), ("team-stealing", 0)])
def test_directed_blocks(form, order):
    jobs = blocks_of(B.directed_cases())
    # the cases whose column does not fit LCAP: 904 is their whole answer here (status 0 / 901 on the GPU tier, which enlarges the workspace)
    assert {c.name for c, _, st, _ in jobs if st == 904} == {"run-of-%d-digits-%s" % (d, w) for d in (19, 20, 21, 22) for w in ("at-the-block-start", "before-eob")} | {
        "BZh1-with-L-of-400100", "one-run-of-2^20", "one-run-of-2^23", "one-run-of-2^25"}
    assert sum(st == 0 for _, _, st, _ in jobs) >= 300
    with stage3(form, order):
        check(jobs, "%s, lane order %d" % (form, order))


@pytest.mark.parametrize("form", list(FORMS))
def test_the_walk_finishes_single_cycle_blocks_itself(form):
    """The serial walk of stage 3b takes over whenever the cut walk of stage 3a does not complete -- and would hide one that never
    does (a wrong successor for the segment that ends at origPtr, say).  So: every block whose column is one cycle -- origPtr on a
    mark and off one, every size of the segment geometry -- comes out of stage 3a, and no block of several cycles does."""
    import ctypes as C
    counter = E.lib.emu_bzip2_fused_finished if form == "fused" else E.lib.emu_bzip2_team_finished
    counter.restype = C.c_uint64
    ok = [x for x in blocks_of(B.directed_cases()) if x[2] == 0 and x[0].block_cycles[x[1]] is not None]
    for single in (True, False):
        jobs = [x for x in ok if (x[0].block_cycles[x[1]] == 1) == single]
        assert len(jobs) >= 100 and any(c.name == "origPtr-off-a-mark" for c, _, _, _ in jobs) == single
        counter(1)
        with stage3(form):
            check(jobs, form)
        assert counter(1) == (len(jobs) if single else 0), (form, single)


@pytest.mark.parametrize("form", list(FORMS))
def test_one_byte_less_than_the_output_needs(form):
    """Every fifth status-0 block at capacity - 1: 901, the length the output needs, and the bytes that fit."""
    ok = [x for x in blocks_of(B.directed_cases()) if x[2] == 0 and len(x[3]) >= 1]
    jobs = ok[::5] + [x for i, x in enumerate(ok) if i % 5 and x[0].name.startswith(("rle1-50000-of-aaaa-ff", "rle1-cut-points", "rle1-no-safe"))]
    assert len(jobs) >= 60 and sum(len(p) == 2590000 for _, _, _, p in jobs) == 1
    with stage3(form):
        res = run(jobs, [len(p) - 1 for _, _, _, p in jobs])
    for (c, j, _, plain), r in zip(jobs, res):
        assert r[0] == 901 and r[3] == len(plain) and r[1] == plain[:-1], "%s, block %d (%s): status %d" % (c.name, j, form, r[0])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("seed", range(3))
def test_random_blocks(seed, form):
    if seed not in _random:          # (built once per seed, shared by the three forms, never changed)
        rnd = random.Random(0xB21B + seed)
        _random[seed] = [B.random_stream(rnd, i % 2 == 0, name="random-%d-%d" % (seed, i), big=i % 16 == 1) for i in range(40)]
    with stage3(form, 2):
        check(blocks_of(_random[seed]), "%s, seed %d" % (form, seed))
