"""GPU tier: bzip2 marks found by a device scan.  swc_batch_bzip2_index against the statement of the mark rule in
tests/_bzip2_marks_cases.py (the case list of the CPU tier), and the bzip2 decoders with "bzip2_scan_bytes" > 0 against the oracle and
against their own result with the knob at 0: the same status, bytes, in_consumed and sizes, whatever the file, with the scan
counters moving by what the rule predicts."""
import bz2
import contextlib
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import _bzip2_build as B
import _bzip2_marks_cases as K
import _oracle as O
import swcompression_amd as swc
from swcompression_amd import _lib, batch, corpus
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu

TILE = 16384   # csrc/gzip_scan.h kTile: test_tile_is_what_the_cases_assume holds the library to it
CASES = K.all_cases(TILE)
WANT = {name: K.rule(b) for name, b in CASES}
SWC_E_INVALID_ARGUMENT, SWC_E_NEED_WORKSPACE = 903, 904   # include/swc_status.h
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return _lib.load()


@contextlib.contextmanager
def scan(lib, least):
    assert lib.swc_set_tuning(b"bzip2_scan_bytes", int(least)) == 0
    try:
        yield
    finally:
        assert lib.swc_set_tuning(b"bzip2_scan_bytes", 0) == 0


def stats(lib):
    return {k: lib.swc_stat(k.encode()) for k in ("bzip2_scan_files", "bzip2_scan_marks", "launches")}


def moved(lib, before):
    now = stats(lib)
    return {k: now[k] - before[k] for k in now}


# ---- the device call ----------------------------------------------------------------------------------------------------------------
def device_index(lib, data, cap, residue=0, room=None, ws_short=0):
    """swc_batch_bzip2_index of `data` at `residue` bytes past a 16-byte boundary, GUARD bytes of 0xA5 around it; the refs 8 bytes past a
    16-byte boundary in `room` refs (default cap) between guards, *n between guards.  Returns (status, n, refs); asserts that nothing
    but the first min(n, cap) refs changed.  ws_short: the workspace is said to be that many bytes smaller than it has to be."""
    import torch
    room = cap if room is None else room
    src = torch.full((GUARD + 16 + len(data) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    at = GUARD + residue
    assert src.data_ptr() % 16 == 0
    if data:
        src[at:at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.full((GUARD + 8 + room * 32 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    n = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    need = lib.swc_bzip2_index_workspace_bytes(len(data), cap)
    ws = torch.full((need + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    opts = _lib.SwcBatchOpts(-1, torch.cuda.current_stream().cuda_stream, 1, 0)
    st = lib.swc_batch_bzip2_index(src.data_ptr() + at, len(data), out.data_ptr() + GUARD + 8, cap, n.data_ptr() + 8, ws.data_ptr(),
                                   need - ws_short, C.byref(opts))
    torch.cuda.synchronize()
    host, n_host, src_host = out.cpu().numpy().tobytes(), n.cpu().numpy(), src.cpu().numpy().tobytes()
    assert src_host[:at] == b"\xa5" * at and src_host[at + len(data):] == b"\xa5" * (len(src_host) - at - len(data)) and src_host[at:at + len(data)] == data
    assert n_host[0] == 0x5A5A5A5A5A5A5A5A and n_host[2] == 0x5A5A5A5A5A5A5A5A
    if st != 0:
        assert host == b"\xa5" * len(host) and n_host[1] == 0x5A5A5A5A5A5A5A5A, "a failed call wrote something"
        assert ws.cpu().numpy().tobytes() == b"\xa5" * (need + 32), "a failed call wrote to its workspace"
        return st, None, None
    found = int(n_host[1])
    m = min(found, cap)
    lo = GUARD + 8
    assert host[:lo] == b"\xa5" * lo and host[lo + 32 * m:] == b"\xa5" * (len(host) - lo - 32 * m), "written outside refs[0, min(n, cap))"
    assert ws.cpu().numpy().tobytes()[need:] == b"\xa5" * 32, "written behind the workspace"
    raw = np.frombuffer(host[lo:lo + 32 * m], dtype=np.dtype([("o", "<u8"), ("c", "<u8"), ("u", "<u8"), ("a", "<u4"), ("f", "<u4")]))
    return st, found, [tuple(int(x) for x in r) for r in raw]


@pytest.mark.parametrize("residue", range(16))
def test_device_index_equals_the_rule(lib, residue):
    """Every case of the CPU tier's list at THIS residue."""
    for name, b in CASES:
        want = WANT[name]
        st, n, refs = device_index(lib, b, len(want) + 1, residue)
        assert (st, n) == (0, len(want)), name
        assert refs == want, name


def test_tile_is_what_the_cases_assume(lib):
    """The workspace is 12 bytes per tile, 8 per slot and 8 to align: a buffer that ends 15 bytes in front of TILE is one tile at any
    alignment, one byte more may be two -- so TILE is the library's kTile, and the border cases are on its borders.  The cases
    themselves are what their names say (the assertions of the CPU tier, on the rule)."""
    assert lib.swc_bzip2_index_workspace_bytes(TILE - 15, 0) == 8 + 8 + 8 + 8
    assert lib.swc_bzip2_index_workspace_bytes(TILE - 14, 0) == 16 + 8 + 8 + 8
    for name, border in (("chunk borders", 16), ("step borders", 1024), ("tile borders", TILE)):
        assert {(r[0] % 8, -(r[0] // 8) % border) for r in WANT[name]} == {(s, d) for s in range(8) for d in (1, 3, 6)}, name
    many = WANT["more than 64 tiles"]
    assert {r[0] // 8 // TILE for r in many} == {0, 2, 63, 64, 65, 69, 70} and len(dict(CASES)["more than 64 tiles"]) > 64 * TILE


def test_device_cap_contract(lib):
    for name in K.CAP_CASES:
        b, want = dict(CASES)[name], WANT[name]
        n = len(want)
        assert n >= 2
        for cap in K.caps(n):
            assert device_index(lib, b, cap, 9, room=cap + 6) == (0, n, want[:cap]), (name, cap)


def test_workspace_and_null_pointers(lib):
    import torch
    b = dict(CASES)["step borders"]
    assert device_index(lib, b, 100, 3, ws_short=1)[0] == SWC_E_NEED_WORKSPACE
    assert device_index(lib, b, 100, 3, ws_short=0)[0] == 0
    assert device_index(lib, b"", 4, 0) == (0, 0, [])
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, opts = t.data_ptr(), _lib.SwcBatchOpts(-1, None, 1, 0)
    need = lib.swc_bzip2_index_workspace_bytes(100, 4)
    assert need <= 2048
    good = [p, 100, p + 1024, 4, p + 2000, p + 2048, need, C.byref(opts)]
    for null in (0, 2, 4, 5):
        args = list(good)
        args[null] = None
        assert lib.swc_batch_bzip2_index(*args) == SWC_E_INVALID_ARGUMENT, null
    torch.cuda.synchronize()
    assert bool((t == 0).all())


def test_python_index_and_a_batch_from_its_rows(lib):
    """batch.bzip2_mark_index on a real stream; the block rows as DeviceBatch("bzip2_block") units decode to the text."""
    import torch
    text = corpus.p_text(250000, 41)
    z = bz2.compress(text, 1)
    want = K.rule(z)
    assert [r[4] for r in want] == [0, 0, 0, 1]
    src = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    n, refs = batch.bzip2_mark_index(src)
    assert n == len(want) and refs.is_cuda and tuple(refs.shape) == (n, 4)
    rows = refs.cpu().tolist()
    assert [tuple(r) for r in rows] == [(o, c, u, a + (f << 32)) for o, c, u, a, f in want]
    n2, refs2 = batch.bzip2_mark_index(src, cap=2)
    assert n2 == n and refs2.cpu().tolist() == rows[:2]
    blocks = [r for r in rows if r[3] < (1 << 32)]
    b = DeviceBatch("bzip2_block", [z] * len(blocks), [100000 + 64] * len(blocks), extra=[r[0] + 80 for r in blocks], dict_values=[r[3] for r in blocks])
    b.launch(sync=True)
    r = b.results()
    assert (r["status"] == 0).all()
    assert b"".join(b.output(i) for i in range(len(blocks))) == text


# ---- the host calls -------------------------------------------------------------------------------------------------------------------
def decompress(lib, data):
    """swc_bzip2_decompress: (status, bytes, in_consumed)."""
    out, n, used = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_size_t(0xEEEE)
    st = lib.swc_bzip2_decompress(bytes(data), len(data), C.byref(out), C.byref(n), C.byref(used))
    blob = C.string_at(out, n.value) if n.value else b""
    lib.swc_free(out)
    return st, blob, used.value


def multi(lib, data):
    """swc_bzip2_multi_decompress: (status, [parts])."""
    out, n, sizes, cnt = C.POINTER(C.c_uint8)(), C.c_size_t(), C.POINTER(C.c_size_t)(), C.c_size_t()
    st = lib.swc_bzip2_multi_decompress(bytes(data), len(data), C.byref(out), C.byref(n), C.byref(sizes), C.byref(cnt))
    blob = C.string_at(out, n.value) if n.value else b""
    szs = [sizes[i] for i in range(cnt.value)]
    lib.swc_free(out)
    lib.swc_free(sizes)
    assert sum(szs) == len(blob)
    parts, o = [], 0
    for s in szs:
        parts.append(blob[o:o + s])
        o += s
    return st, parts


def predicted(data, least=1):
    """How the counters move for one archive: (files, marks)."""
    if len(data) < max(least, 14):   # (no buffer under 14 bytes holds a mark: nothing to stage)
        return 0, 0
    return 1, sum(1 for r in K.rule(data) if r[4] == 0)


def both_ways(lib, call, data):
    """`call` with the knob at 1 and at 0: the same result; the counters move by what the rule predicts with it, not at all without."""
    before = stats(lib)
    with scan(lib, 1):
        got = call(lib, data)
    d = moved(lib, before)
    files, marks = predicted(data)
    assert (d["bzip2_scan_files"], d["bzip2_scan_marks"]) == (files, marks), d
    before = stats(lib)
    plain = call(lib, data)
    d0 = moved(lib, before)
    assert d0["bzip2_scan_files"] == 0 and d0["bzip2_scan_marks"] == 0, d0
    assert got == plain, "the knob changes the result"
    assert d["launches"] >= d0["launches"]
    return got


def as_the_oracle(lib, data):
    st, out, used = both_ways(lib, decompress, data)
    est, eout, eused = O.bzip2(data)
    assert st == est
    assert out == (eout if est in (0, 210) else b"")   # (only wrongCRC carries data)
    if est == 0:
        assert used == eused
    mst, parts = both_ways(lib, multi, data)
    est, eparts = O.bzip2_multi(data)
    assert mst == est and parts == (eparts if est in (0, 210) else [])
    return st, out


@functools.lru_cache(maxsize=None)
def three_blocks():
    text = corpus.p_text(250000, 43)
    z = bz2.compress(text, 1)
    marks = K.rule(z)
    assert [r[4] for r in marks] == [0, 0, 0, 1]
    return text, z, marks


def test_clean_streams(lib):
    text, z, _ = three_blocks()
    assert as_the_oracle(lib, z) == (0, text)
    two = z + bz2.compress(text[:5000], 9) + bz2.compress(b"", 5) + bz2.compress(text[5000:130000], 1)
    assert as_the_oracle(lib, two) == (0, text)
    assert both_ways(lib, multi, two) == (0, [text, text[:5000], b"", text[5000:130000]])
    for data in (b"", b"BZh9", b"BZh91AY&SY", z[:13], z[:14]):
        as_the_oracle(lib, data)


@pytest.fixture
def output_cap():
    """The oracle's output cap where the built set expects it (a run of 2^25 is 901 on both sides), as tests/test_gpu_bzip2_built.py."""
    O.lib.refcpu_set_max_output(B.MAX_OUTPUT)
    yield
    O.lib.refcpu_set_max_output(1 << 30)


SLICES = 16


@pytest.mark.parametrize("k", range(SLICES))
def test_built_streams_one_by_one(lib, output_cap, k):
    """Every directed case of tests/_bzip2_build.py by swc_bzip2_decompress, clean and damaged, the runs that take a block through
    several launches among them (every SLICES-th case from k on)."""
    cases = B.directed_cases()
    assert len(cases) >= 400 and sum(1 for c in cases if c.status != 0) >= 25
    for c in cases[k::SLICES]:
        st, out, used = both_ways(lib, decompress, c.stream)
        est, eout, eused = O.bzip2(c.stream)
        assert st == est == c.status, c.name
        assert out == (eout if est in (0, 210) else b""), c.name
        assert est != 0 or used == eused, c.name


def test_built_streams_back_to_back(lib):
    for name, data in B.multi_cases():
        assert as_the_oracle(lib, data)[0] == 0, name


RELAUNCH = ("BZh1-with-L-of-", "one-run-of-2^1", "one-run-of-2^20", "one-run-of-2^23")   # (a block comes back for a larger workspace)
GROUPS = {"to-70000": lambda c: not c.name.startswith(RELAUNCH) and max(c.l_len) <= 70000,
          "longer": lambda c: not c.name.startswith(RELAUNCH) and max(c.l_len) > 70000,
          "relaunched": lambda c: c.name.startswith(RELAUNCH)}


def test_the_groups_hold_every_clean_case():
    clean = [c for c in B.directed_cases() if c.status == 0]
    assert len(clean) >= 380 and all(sum(1 for g in GROUPS.values() if g(c)) == 1 for c in clean)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_built_streams_in_one_call(lib, group):
    """The clean directed cases -- ALL of them over the three groups, which only keep each test short -- in ONE swc_unarchive_many with
    the knob on: every archive of 14 bytes and more is indexed on the device and stays in HBM until the launches have read it, the
    blocks that come back for a larger workspace too."""
    clean = [c for c in B.directed_cases() if c.status == 0 and GROUPS[group](c)]
    assert len(clean) >= (300 if group == "to-70000" else 5)
    before = stats(lib)
    with scan(lib, 1):
        got = swc.unarchive_many("bzip2", [c.stream for c in clean])
    d = moved(lib, before)
    want = [predicted(c.stream) for c in clean]
    assert (d["bzip2_scan_files"], d["bzip2_scan_marks"]) == (sum(f for f, _ in want), sum(m for _, m in want)), d
    assert [g[0] for g in got] == [0] * len(clean)
    for c, g in zip(clean, got):
        assert g[1] == c.plain, c.name


def test_damaged_and_truncated(lib):
    text, z, marks = three_blocks()
    second = marks[1][0]
    crc = bytearray(z)   # the stored CRC of the second block: it decodes, and does not match
    crc[(second + 60) >> 3] ^= 0x10
    st, out = as_the_oracle(lib, bytes(crc))
    assert st == 210 and 150000 < len(out) < len(text) and text.startswith(out)   # wrongCRC: everything so far, the block itself too
    body = bytearray(z)   # a bit in the second block's data: whatever the oracle makes of it
    body[(second >> 3) + 5000] ^= 0x04
    assert as_the_oracle(lib, bytes(body))[0] != 0
    in_block = z[:(marks[2][0] >> 3) + 3000]
    assert as_the_oracle(lib, in_block)[0] != 0
    end = marks[3][0] >> 3
    for cut in (end + 1, end + 5, end + 9, len(z) - 1):   # inside the end mark: in its magic, in its word
        assert as_the_oracle(lib, z[:cut])[0] != 0
    total = bytearray(z)
    total[-2] ^= 0x80   # the combined CRC
    assert as_the_oracle(lib, bytes(total))[0] == 210


def test_magic_behind_the_end_of_the_stream(lib):
    """A block magic in bytes the walk never arrives at: a mark, a unit -- and no part of the result."""
    text, z, marks = three_blocks()
    tail = K.noise(3000, 77)
    K.plant(tail, 8 * 1000 + 3)
    data = z + bytes(tail)
    assert sum(1 for r in K.rule(data) if r[4] == 0) == 4
    st, out, used = both_ways(lib, decompress, data)
    assert (st, out, used) == (0, text, len(z)) == O.bzip2(data)
    both_ways(lib, multi, data)   # (the walk goes on into the noise: an error, the same both ways)
    assert multi(lib, data)[0] == O.bzip2_multi(data)[0] != 0


def test_more_marks_than_the_first_call_has_room_for(lib):
    """BZh9 and 5,000 bare marks 80 bits apart -- every fiftieth a block's, the others ends of streams: over the 4,096 the first
    index call has room for, so a second one with room for all; the walk meets the first mark, the end of an empty stream."""
    data = bytearray(b"BZh9")
    for i in range(5000):
        data += (K.BLOCK if i % 50 == 7 else K.END).to_bytes(6, "big") + struct.pack(">I", 0 if i == 0 else 0xA0000000 + i)
    data = bytes(data)
    want = K.rule(data)
    assert len(want) == 5000 and sum(1 for r in want if r[4] == 0) == 100
    before = stats(lib)
    with scan(lib, 1):
        got = decompress(lib, data)
    d = moved(lib, before)
    assert got == (0, b"", 14) == O.bzip2(data)
    assert (d["bzip2_scan_files"], d["bzip2_scan_marks"]) == (1, 100), d
    before = stats(lib)
    assert decompress(lib, data) == got
    d0 = moved(lib, before)
    assert d["launches"] == d0["launches"] + 2 and d0["bzip2_scan_files"] == 0 and d0["bzip2_scan_marks"] == 0, (d, d0)   # (the two index calls)


def test_unarchive_many_around_the_knob(lib):
    """One archive below the knob's size and two above it: the two are scanned on the device, the results are the oracle's."""
    text, z, marks = three_blocks()
    small = bz2.compress(text[:300], 9)
    other = bz2.compress(text[100000:180000], 1)
    damaged = bytearray(other)
    damaged[12] ^= 1   # (the first block's stored CRC)
    archives = [z, small, bytes(damaged)]
    assert len(small) < 3000 < len(other)
    before = stats(lib)
    with scan(lib, 3000):
        got = swc.unarchive_many("bzip2", archives)
    d = moved(lib, before)
    assert (d["bzip2_scan_files"], d["bzip2_scan_marks"]) == (2, 3 + 1), d
    before = stats(lib)
    assert swc.unarchive_many("bzip2", archives) == got
    d0 = moved(lib, before)
    assert d0["bzip2_scan_files"] == 0 and d0["bzip2_scan_marks"] == 0 and d["launches"] == d0["launches"] + 2, (d, d0)
    for a, (st, out) in zip(archives, got):
        est, eout = O.bzip2(a)[:2]
        assert st == est and out == (eout if est in (0, 210) else b"")
    assert [st for st, _ in got] == [0, 0, 210]
