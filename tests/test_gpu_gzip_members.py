"""GPU tier: plain gzip members found by a device scan.  swc_batch_gzip_index against the statement of the candidate rule in
tests/_gzip_members_cases.py (the case list of the CPU tier), and swc_gzip_multi_unarchive with "gzip_member_scan" = 1 against the
oracle: the same status and the same parts, whatever the file, with the members taken from ONE launch where the file is clean."""
import contextlib
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import _gzip_members_cases as K
import _oracle as O
from swcompression_amd import _lib, batch, corpus

pytestmark = pytest.mark.gpu

TILE = 16384   # csrc/gzip_scan.h kTile (the CPU tier asks the emulation; the sizes here only have to cross it)
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
def scan(lib, on):
    assert lib.swc_set_tuning(b"gzip_member_scan", int(on)) == 0
    try:
        yield
    finally:
        assert lib.swc_set_tuning(b"gzip_member_scan", 0) == 0


def stats(lib):
    return {k: lib.swc_stat(k.encode()) for k in ("gzip_scan_members", "gzip_scan_walked", "launches")}


def moved(lib, before):
    now = stats(lib)
    return {k: now[k] - before[k] for k in now}


# ---- the device call ----------------------------------------------------------------------------------------------------------------
def device_index(lib, data, cap, residue=0, room=None, ws_short=0):
    """swc_batch_gzip_index of `data` at `residue` bytes past a 16-byte boundary, GUARD bytes of 0xA5 around it; the refs 8 bytes past a
    16-byte boundary in `room` refs (default cap) between guards.  Returns (status, n, refs); asserts that nothing but the first min(n,
    cap) refs changed.  ws_short: the workspace is said to be that many bytes smaller than it has to be."""
    import torch
    room = cap if room is None else room
    src = torch.full((GUARD + 16 + len(data) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    at = GUARD + residue
    assert src.data_ptr() % 16 == 0
    if data:
        src[at:at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.full((GUARD + 8 + room * 32 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    n = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    need = lib.swc_gzip_index_workspace_bytes(len(data), cap)
    ws = torch.full((need + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    opts = _lib.SwcBatchOpts(-1, torch.cuda.current_stream().cuda_stream, 1, 0)
    st = lib.swc_batch_gzip_index(src.data_ptr() + at, len(data), out.data_ptr() + GUARD + 8, cap, n.data_ptr() + 8, ws.data_ptr(),
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
    """Every case of the CPU tier's list: the lengths 0..44 and those around one and two tiles at THIS residue, the others at this
    residue too."""
    for name, b in CASES:
        want = WANT[name]
        st, n, refs = device_index(lib, b, len(want) + 1, residue)
        assert (st, n) == (0, len(want)), name
        assert refs == want, name


def test_device_cap_contract(lib):
    for name in ("soak 0", "dense 1027", "flags 1f", "length %d" % (TILE + 7)):
        b, want = dict(CASES)[name], WANT[name]
        n = len(want)
        assert n >= 2
        for cap in (0, 1, n - 1, n, n + 1):
            assert device_index(lib, b, cap, 9, room=cap + 3) == (0, n, want[:cap]), (name, cap)


def test_workspace_and_null_pointers(lib):
    import torch
    b = dict(CASES)["soak 1"]
    assert device_index(lib, b, 100, 3, ws_short=1)[0] == SWC_E_NEED_WORKSPACE
    assert device_index(lib, b, 100, 3, ws_short=0)[0] == 0
    assert device_index(lib, b"", 4, 0) == (0, 0, [])
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, opts = t.data_ptr(), _lib.SwcBatchOpts(-1, None, 1, 0)
    need = lib.swc_gzip_index_workspace_bytes(100, 4)
    assert need <= 2048
    good = [p, 100, p + 1024, 4, p + 2000, p + 2048, need, C.byref(opts)]
    for null in (0, 2, 4, 5):
        args = list(good)
        args[null] = None
        assert lib.swc_batch_gzip_index(*args) == SWC_E_INVALID_ARGUMENT, null
    torch.cuda.synchronize()
    assert bool((t == 0).all())


def test_python_device_index(lib):
    import torch
    b = dict(CASES)["length %d" % (2 * TILE + 3)]
    want = WANT["length %d" % (2 * TILE + 3)]
    src = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    n, refs = batch.gzip_member_index(src)
    assert n == len(want) and refs.is_cuda and tuple(refs.shape) == (n, 4)
    assert [tuple(r) for r in refs.cpu().tolist()] == [(o, c, u, a + (f << 32)) for o, c, u, a, f in want]
    n2, refs2 = batch.gzip_member_index(src, cap=2)
    assert n2 == n and refs2.cpu().tolist() == refs[:2].cpu().tolist()


# ---- the host call --------------------------------------------------------------------------------------------------------------------
def gz(payload, flags=0, raw=None, name=b"member.txt", comment=b"a comment", level=6):
    """A gzip member with the header fields `flags` asks for, all of them as the reference accepts them."""
    h = bytes([0x1f, 0x8b, 8, flags]) + struct.pack("<I", 1700000000) + b"\x00\x03"
    if flags & 4:
        h += struct.pack("<H", 8) + b"Ap" + struct.pack("<H", 4) + b"data"
    if flags & 8:
        h += name + b"\0"
    if flags & 16:
        h += comment + b"\0"
    if flags & 2:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + (corpus.deflate_raw(payload, level) if raw is None else raw) + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload) & 0xFFFFFFFF)


def payloads(n, top=4096, seed=0):
    rng = np.random.Generator(np.random.PCG64(0x6A1B + seed))
    kinds = (corpus.p_text, corpus.p_mix, corpus.p_rand, corpus.p_rep)
    return [b"" if i % 37 == 5 else kinds[i % 4](int(rng.integers(0, top + 1)), 4000 + seed * 1000 + i) for i in range(n)]


def multi(lib, data):
    """swc_gzip_multi_unarchive as the oracle's wrapper returns it: (status, [parts])."""
    out, n, sizes, cnt = C.POINTER(C.c_uint8)(), C.c_size_t(), C.POINTER(C.c_size_t)(), C.c_size_t()
    st = lib.swc_gzip_multi_unarchive(bytes(data), len(data), C.byref(out), C.byref(n), C.byref(sizes), C.byref(cnt))
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


def scanned(lib, data):
    """The call with the knob on: (what it returned, how the counters moved) -- and what it returned is what the oracle returns."""
    before = stats(lib)
    with scan(lib, 1):
        got = multi(lib, data)
    d = moved(lib, before)
    st, parts = O.gzip_multi_unarchive(data)
    # (GzipError.wrongCRC carries the members so far, no other error carries anything: the oracle's wrapper hands back whatever its
    # buffer held, the library nothing -- as tests/test_gpu_many.py reads the two)
    assert got == (st, parts if st in (0, 605) else [])
    assert got == multi(lib, data), "the walk alone returns something else"
    return got, d


def test_clean_file_is_one_launch(lib):
    """200 clean members of 0..4 KiB, every flag combination among the headers: all taken from the launch ahead, none walked, two
    launches at the most (the index, the members); with the knob off: the counters stand still, a launch per member."""
    parts = payloads(200)
    data = b"".join(gz(p, i % 32) for i, p in enumerate(parts))
    assert len(K.rule(data)) == 200 and not any(r[4] for r in K.rule(data))   # (no candidate but the members)
    (st, got), d = scanned(lib, data)
    assert st == 0 and got == parts
    assert d["gzip_scan_members"] == 200 and d["gzip_scan_walked"] == 0 and d["launches"] <= 2, d
    before = stats(lib)
    with scan(lib, 0):
        assert multi(lib, data) == (0, parts)
    d = moved(lib, before)
    assert d["gzip_scan_members"] == 0 and d["gzip_scan_walked"] == 0 and d["launches"] >= 200, d


def test_nested_file(lib):
    """One of 20 members is a stored block whose payload is a complete .gz file: the candidate inside it cuts that member short, the walk
    decodes exactly that one itself."""
    parts = payloads(20, seed=1)
    parts[11] = gz(corpus.p_text(3000, 77), 8) + gz(b"second inner member")
    members = [gz(p, i % 32) for i, p in enumerate(parts)]
    inner = parts[11]
    members[11] = gz(inner, 0, raw=b"\x01" + struct.pack("<HH", len(inner), len(inner) ^ 0xFFFF) + inner)
    (st, got), d = scanned(lib, b"".join(members))
    assert st == 0 and got == parts
    assert d["gzip_scan_walked"] == 1 and d["gzip_scan_members"] == 19, d


def test_name_over_the_limit(lib):
    parts = payloads(20, seed=2)
    members = [gz(p, i % 32) for i, p in enumerate(parts)]
    members[4] = gz(parts[4], 8, name=b"n" * 299)
    (st, got), d = scanned(lib, b"".join(members))
    assert st == 0 and got == parts
    assert d["gzip_scan_walked"] == 1 and d["gzip_scan_members"] == 19, d


def _twenty(seed):
    parts = payloads(20, top=3000, seed=seed)
    parts[7] = corpus.p_text(2500, 7)
    return parts, [gz(p, (i * 7) % 32) for i, p in enumerate(parts)]


def test_wrong_crc_carries_the_members_so_far(lib):
    parts, members = _twenty(3)
    m = bytearray(members[7])
    m[-8] ^= 0x40
    members[7] = bytes(m)
    (st, got), d = scanned(lib, b"".join(members))
    assert st != 0 and got == parts[:8]
    assert d["gzip_scan_members"] == 7 and d["gzip_scan_walked"] == 1, d


def test_wrong_isize(lib):
    parts, members = _twenty(4)
    m = bytearray(members[7])
    m[-4:] = struct.pack("<I", len(parts[7]) + 1)
    members[7] = bytes(m)
    (st, got), d = scanned(lib, b"".join(members))
    assert st != 0 and got == []


@pytest.mark.parametrize("cut", range(1, 13))
def test_last_member_truncated(lib, cut):
    parts, members = _twenty(5)
    data = b"".join(members)[:-cut]
    (st, got), d = scanned(lib, data)
    assert st != 0
    assert d["gzip_scan_members"] == 19, d


def test_garbage_behind_the_last_member(lib):
    parts, members = _twenty(6)
    (st, got), d = scanned(lib, b"".join(members) + b"\x00\x1f\x8b\x08\x00")
    assert st != 0 and got == []
    assert d["gzip_scan_members"] == 19 and d["gzip_scan_walked"] == 1, d   # (the last member's unit ran to the end of the file: the walk took it)


def test_reserved_flag_at_member_3(lib):
    parts, members = _twenty(7)
    m = bytearray(members[3])
    m[3] |= 0x20
    members[3] = bytes(m)
    (st, got), d = scanned(lib, b"".join(members))
    assert st != 0 and got == []
    assert d["gzip_scan_members"] == 2 and d["gzip_scan_walked"] == 1, d   # (member 2's unit ran on into member 3: the walk took it)


def test_single_members(lib):
    p = corpus.p_text(3000, 1)
    (st, got), d = scanned(lib, gz(p, 8))
    assert (st, got) == (0, [p]) and d["gzip_scan_members"] == 0 and d["gzip_scan_walked"] == 0
    (st, got), d = scanned(lib, gz(p, 0) + b"\x00" * 19)
    assert st != 0 and d["gzip_scan_members"] == 0 and d["gzip_scan_walked"] == 0


def test_bgzf_still_takes_its_own_launch(lib):
    parts = payloads(30, seed=8)
    data = b"".join(corpus.gzip_member(p, bgzf=True) for p in parts)
    (st, got), d = scanned(lib, data)
    assert st == 0 and got == parts
    assert d["gzip_scan_members"] == 0 and d["gzip_scan_walked"] == 0 and d["launches"] == 1, d
