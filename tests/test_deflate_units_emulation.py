"""CPU tier of the Deflate units: phase 1 with the OPEN rule (csrc/inflate_sync.h), the placing scan (csrc/deflate_place.h) and the
copy at any byte address (csrc/lz_copy.h, lz_resolve.h) in the host emulation, under the three lane orders, against units built
code by code (_deflate_units_cases) and the oracle; the stand-alone program under ASan + UBSan on the same cases."""
import ctypes as C
import zlib

import pytest

import _deflate_units_cases as K
import _emu
import _emu_deflate_units as E

ORDERS = [0, 1, 2]
RUNS = K.directed_runs()


@pytest.fixture(scope="module")
def expected():
    return {name: [K.expect(u) for u in run] for name, run in RUNS.items()}


def check_run(name, units, exp, got):
    """Every job against what is expected of it, and every joined job right behind what its predecessor says exists."""
    at = 0
    for k, (u, e, g) in enumerate(zip(units, exp, got)):
        what = "%s unit %d" % (name, k)
        st, n, cons, aux, out = e
        gst, gn, gcons, gaux, rel, gout = g
        assert gst == st, what
        assert gaux == aux, what + ": aux"
        assert rel == at, what + ": not placed behind its predecessor"
        if n is not None:
            assert (gn, gcons) == (n, cons), what
            assert gout == out, what
        at += min(gn, u["cap"])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("copier,team", [(1, 0), (0, 0), (1, 1)])
def test_directed_runs(expected, order, copier, team):
    """All runs as ONE job list: an open unit behind an empty stored block, one that ends after a fixed block exactly on a byte, the
    same one code longer (a plain job's status), one with a final block and bytes behind it, a unit that reaches back, a middle unit
    over capacity, empty units."""
    E.set_order(order)
    try:
        units = [u for run in RUNS.values() for u in run]
        got = E.run_units(units, copier=copier, team=team)
    finally:
        E.set_order(0)
    i = 0
    for name, run in RUNS.items():
        check_run(name, run, expected[name], got[i:i + len(run)])
        i += len(run)
    assert expected["one-code-longer"][0][0] not in (K.OK,)
    assert expected["reaches-back"][1][0] == K.REF_TRAP
    assert expected["over-capacity"][1][:2] == (K.CAPACITY, 1501)


def test_plain_jobs_unchanged():
    """aux = 0: an open-ended unit is the truncated stream it always was (SWC_E_REF_TRAP at the missing block header)."""
    run = RUNS["stored-markers"]
    got = E.run_units([dict(u, aux=0, open_plain=None) for u in run[:1]])
    assert got[0][0] == K.REF_TRAP and got[0][3] == 0


def test_joined_job_0():
    """SWC_DEFLATE_JOINED on job 0 (and on what is joined to it): SWC_E_INVALID_ARGUMENT, nothing produced; the next head is untouched."""
    run = RUNS["stored-markers"]
    units = [dict(run[1]), dict(run[2]), dict(run[0]), dict(run[2])]
    got = E.run_units(units)
    for g in got[:2]:
        assert g[:3] == (K.INVALID_ARGUMENT, 0, 0)
    check_run("behind the orphans", units[2:], [K.expect(u) for u in units[2:]], got[2:])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("rev", [False, True])
def test_place_scan(order, rev):
    """The scan alone: a run of 200 units of 300 bytes (crosses three tile borders), two runs inside one tile, sizes 1 / 0 / 70,001,
    over-capacity sizes, a run that ends with the list; jobs that are not joined keep their `out`, nobody's status is touched."""
    E.set_order(order)
    sizes = [300] * 200 + [17, 5, 9] + [40, 41] + [1, 0, 70001, 0, 1] + [5000, 10, 3]
    caps = [300] * 200 + [17, 5, 9] + [64, 64] + [1, 1, 70001, 8, 1] + [100, 10, 3]
    aux = [0] + [3] * 198 + [1] + [2, 3, 1] + [2, 1] + [2, 3, 3, 3, 1] + [0, 3, 1]
    try:
        got = E.place(sizes, caps, aux, reversed_=rev)
    finally:
        E.set_order(0)
    head, at = None, 0
    for i, (out, st, n) in enumerate(got):
        assert st == 902 and n == sizes[i]
        if not aux[i] & K.JOINED:
            head, at = out, 0
            assert out == 0x10000 + (i << 32)
        assert out == head + at, "job %d" % i
        at += min(sizes[i], caps[i])


def test_place_scan_orphans():
    """Joined jobs with no head: a whole tile of them and the start of the next; the run behind them is placed."""
    n = 70
    got = E.place([10] * (n + 3), [10] * (n + 3), [1] * n + [0, 1, 1])
    assert all(g == (0, K.INVALID_ARGUMENT, 0) for g in got[:n])
    base = got[n][0]
    assert [g[0] - base for g in got[n:]] == [0, 10, 20] and all(g[1] == 902 for g in got[n:])


@pytest.mark.parametrize("copier", [1, 0])
@pytest.mark.parametrize("rev", [False, True])
def test_copy_at_every_residue(copier, rev):
    """Adjacent units whose seam lies at each of the 16 residues, at each of the 16 residues of the head, copied in both orders: both
    outputs exact -- whichever is written second leaves the line it shares with its neighbour intact -- and the 16 guard bytes on both
    sides untouched (asserted by run_units)."""
    pairs = K.residue_pairs()
    exp = [[K.expect(u) for u in run] for run in pairs]
    for mis in range(16):
        units = [u for run in pairs for u in run]
        got = E.run_units(units, misalign=mis, copier=copier, reversed_=rev)
        for r, run in enumerate(pairs):
            check_run("residue %d at %d" % (r, mis), run, exp[r], got[2 * r:2 * r + 2])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("copier,rev", [(1, False), (0, True)])
def test_long_run_across_tiles(order, copier, rev):
    """A run of 150 units that starts at job 37 and crosses two tile borders, sizes unlike capacities (a 0, a 1, one over capacity):
    decoded, placed and copied; every unit right behind what its predecessor says exists."""
    E.set_order(order)
    jobs = K.long_run()
    exp = [K.expect(u) for u in jobs]
    try:
        got = E.run_units(jobs, misalign=5, copier=copier, reversed_=rev)
    finally:
        E.set_order(0)
    assert [e[0] for e in exp[37:187]].count(K.CAPACITY) == 1 and exp[37 + 20][1] == 0 and exp[37 + 70][1] == 1
    for i in range(37):
        check_run("whole stream %d" % i, jobs[i:i + 1], exp[i:i + 1], got[i:i + 1])
    check_run("the long run", jobs[37:187], exp[37:187], got[37:187])
    check_run("the run behind it", jobs[187:], exp[187:], got[187:])
    assert got[186][4] != sum(u["cap"] for u in jobs[37:186])      # not where the capacities alone would put it


CRC_GROUP_LEN = 1 << 20   # csrc/job_kernels.h: kCrcGroupLen
SENTINEL = 0xA5A5A5A5


def zeros_stream(n):
    z = zlib.compressobj(9, zlib.DEFLATED, -15)
    return K.U(z.compress(bytes(n)) + z.flush(), n, 0)


def test_fused_crc(expected):
    """The copy kernel that ends with the CRC-32 of its output: after one launch over the directed runs and the long run, crcs[g] is the
    CRC-32 of the bytes that exist at job g's `out` -- of a failed unit, of a unit over capacity, of an empty one too.  A stream of
    kCrcGroupLen - 1 bytes gets its CRC there; one of kCrcGroupLen bytes is the group kernel's, its word keeps what it held."""
    units = [u for run in RUNS.values() for u in run] + K.long_run() + [zeros_stream(CRC_GROUP_LEN - 1), zeros_stream(CRC_GROUP_LEN)]
    crcs = (C.c_uint32 * len(units))(*[SENTINEL] * len(units))
    got = E.run_units(units, misalign=5, copier=1, crcs=crcs)
    i = 0
    for name, run in RUNS.items():
        check_run(name, run, expected[name], got[i:i + len(run)])
        i += len(run)
    for k, g in enumerate(got[:-1]):
        assert g[5] is not None and crcs[k] == zlib.crc32(g[5]), "unit %d (status %d, out_len %d)" % (k, g[0], g[1])
    assert [(g[0], g[1]) for g in got[-2:]] == [(K.OK, CRC_GROUP_LEN - 1), (K.OK, CRC_GROUP_LEN)]
    assert got[-1][5] == bytes(CRC_GROUP_LEN) and crcs[len(units) - 1] == SENTINEL
    assert any(g[0] not in (K.OK, K.CAPACITY) for g in got) and any(g[0] == K.CAPACITY for g in got) and any(g[0] == K.OK and g[1] == 0 for g in got)


def test_standalone_program_sanitized(tmp_path, expected):
    """tests/host_emu/emu_deflate_units.cpp as a program of its own under ASan + UBSan on the same cases: every directed run (of a
    failed unit the status and aux), JOINED on job 0, residue pairs, the long run across tiles, and the place-scan lists (built into
    the program) -- 16 alignments x 3 lane orders x both copiers x both copy orders, the team instantiation of phase 1 and the CRC form of the copy, in
    allocations of exactly the lines the contract names."""
    cases = [(RUNS[name], expected[name]) for name in RUNS]
    run = RUNS["stored-markers"]
    orphans = [dict(run[1]), dict(run[2])]
    cases.append((orphans + run, [(K.INVALID_ARGUMENT, 0, 0, K.expect(u)[3], b"") for u in orphans]     # (aux as the parse left it)
                  + expected["stored-markers"]))
    for pair in K.residue_pairs()[::5]:
        cases.append((pair, [K.expect(u) for u in pair]))
    long_ = K.long_run()
    cases.append((long_, [K.expect(u) for u in long_]))
    out = _emu.run_program(tmp_path, "emu_deflate_units.cpp", "EMU_DEFLATE_UNITS_MAIN", E.case_file(cases))
    assert "%d cases, 0 mismatches" % len(cases) in out
