"""CPU tier of the BGZF writer: the host build of csrc/bgzf_pack.h (tests/host_emu/emu_bgzf.cpp) -- the offsets and the pack
against a packer written here, at every border alignment and in three thread orders; the capacity rule; whole files from the
emulated compressors read back by gzip, by the host indexer and member by member; the host-only part of the C ABI."""
import ctypes as C
import gzip
import struct
import zlib

import pytest

import _emu as E
import _emu_bgzf as B
import swcompression_amd as swc
from swcompression_amd import _lib, corpus

SWC_E_CAPACITY, SWC_E_INVALID_ARGUMENT = 901, 903
# every length 1..48 once, three members of 28 bytes in a row, and the sizes around a step of the interior loop and at the top
LENGTHS = list(range(1, 49)) + [2, 2, 2, 255, 256, 257, 4093, 65285]


def member(stream, crc, isize):
    """One BGZF member around a Deflate stream (SAM/BAM specification 4.1)."""
    return B.HEADER + struct.pack("<H", 26 + len(stream) - 1) + bytes(stream) + struct.pack("<II", crc, isize)


def reference_pack(streams, crcs, isizes):
    """The packer the device code is compared with: (file, member sizes incl. the end-of-file member)."""
    parts = [member(s, c, n) for s, c, n in zip(streams, crcs, isizes)] + [B.EOF]
    return b"".join(parts), [len(p) for p in parts]


def arbitrary_streams():
    """The pack does not look inside a stream: arbitrary bytes, every member its own."""
    blob = corpus.p_rand(sum(LENGTHS) + 64, 77)
    out, o = [], 0
    for k, n in enumerate(LENGTHS):
        out.append(bytes([(k * 37 + 1) & 0xFF]) + blob[o + 1:o + n])
        o += n
    return out


STREAMS = arbitrary_streams()
CRCS = [(0x9E3779B1 * (k + 1)) & 0xFFFFFFFF for k in range(len(STREAMS))]
ISIZES = [(k * 4099 + 7) & 0xFFFF for k in range(len(STREAMS))]
EXPECTED, EXPECTED_SIZES = reference_pack(STREAMS, CRCS, ISIZES)


def test_member_starts_fall_on_every_destination_alignment():
    offs, o = [], 0
    for s in EXPECTED_SIZES[:-1]:
        offs.append(o)
        o += s
    assert {x % 16 for x in offs} == set(range(16))
    assert [len(s) for s in STREAMS] == LENGTHS and len(EXPECTED) == sum(26 + n for n in LENGTHS) + 28


@pytest.mark.parametrize("order", [0, 1, 2])
def test_scan_and_pack_against_the_python_packer(order):
    B.set_order(order)
    try:
        for mis in range(16):
            st, out, total, sizes, _ = B.pack(STREAMS, CRCS, ISIZES, misalign=mis)   # (B.pack asserts the guards)
            assert st == 0 and total == len(EXPECTED) and sizes == EXPECTED_SIZES
            assert out == EXPECTED, "destination misaligned by %d" % mis
    finally:
        B.set_order(0)


def test_without_the_end_of_file_member_and_with_no_member():
    st, out, total, sizes, _ = B.pack(STREAMS[:50], CRCS[:50], ISIZES[:50], eof=False, misalign=5)
    assert st == 0 and out == EXPECTED[:total] and sizes == EXPECTED_SIZES[:50] and total == sum(EXPECTED_SIZES[:50])
    assert B.pack([], [], []) == (0, B.EOF, 28, [28], 0)
    assert B.pack([], [], [], eof=False)[:4] == (0, b"", 0, [])


def test_capacity_one_byte_short_writes_nothing():
    for mis in (0, 7):
        st, out, total, _, _ = B.pack(STREAMS, CRCS, ISIZES, dst_cap=len(EXPECTED) - 1, misalign=mis)
        assert st == SWC_E_CAPACITY and total == len(EXPECTED)
        assert out == b"\xA5" * (len(EXPECTED) - 1)          # nothing in front of dst_cap either; the guards behind it: B.pack
    st, out, total, _, _ = B.pack(STREAMS[:3], CRCS[:3], ISIZES[:3], dst_cap=0)
    assert st == SWC_E_CAPACITY and total == sum(EXPECTED_SIZES[:3]) + 28


def test_first_compress_error_by_member_index_stops_the_pack():
    streams, crcs, isizes = STREAMS[:48] * 3, CRCS[:48] * 3, ISIZES[:48] * 3      # 144 members: three steps of the scan
    statuses = [0] * len(streams)
    statuses[9], statuses[70] = 901, 902
    st, out, _, _, bad = B.pack(streams, crcs, isizes, statuses=statuses)
    assert (st, bad) == (901, 9) and out == b"\xA5" * len(out)
    statuses[9] = 0
    assert B.pack(streams, crcs, isizes, statuses=statuses)[::4] == (902, 70)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_running_sum_across_the_steps_of_the_scan(order):
    streams, crcs, isizes = STREAMS[:48] * 3 + STREAMS[-1:], CRCS[:48] * 3 + CRCS[-1:], ISIZES[:48] * 3 + ISIZES[-1:]
    expected, sizes = reference_pack(streams, crcs, isizes)
    B.set_order(order)
    try:
        assert B.pack(streams, crcs, isizes, misalign=9) == (0, expected, len(expected), sizes, 0)
    finally:
        B.set_order(0)


def test_setup_cuts_the_input_into_jobs():
    data = corpus.p_text(1000, 3)
    for bs in (1, 37, 999, 1000, 1001):
        p = B.plan(len(data), bs)
        n = p["n"]
        assert n == -(-len(data) // bs) and p["stride"] % 16 == 0 and p["stride"] >= min(bs, len(data)) + min(bs, len(data)) // 8 + 32
        assert p["bytes"] == p["slots"] + n * p["stride"] and p["cjobs"] < p["kjobs"] < p["crcs"] < p["offs"] < p["res"] < p["slots"]
        cj, kj = (E.Job * n)(), (E.Job * n)()
        src = C.create_string_buffer(data, len(data))
        B.lib.emu_bgzf_setup(src, C.c_uint64(len(data)), C.c_uint32(bs), cj, kj, C.c_void_p(4096), C.c_uint64(p["stride"]))
        for i in range(n):
            c = min(bs, len(data) - i * bs)
            assert (cj[i].in_, cj[i].in_len, cj[i].aux) == (C.addressof(src) + i * bs, c, 0)
            assert cj[i].out == 4096 + i * p["stride"] and cj[i].out % 4 == 0
            assert c + c // 8 + 32 <= cj[i].out_cap <= p["stride"]
            assert (kj[i].out, kj[i].out_len, kj[i].out_cap) == (cj[i].in_, c, c)


# ---- end to end on the emulation ------------------------------------------------------------------------------------------------
def chunks_of(data, bs):
    return [data[i:i + bs] for i in range(0, len(data), bs)]


def emu_archive(data, bs, dynamic):
    cs = chunks_of(data, bs)
    res = E.run_batch("emu_deflate_compress_dynamic" if dynamic else "emu_deflate_compress", cs, [len(c) + len(c) // 8 + 32 for c in cs]) if cs else []
    assert all(r[0] == 0 for r in res)
    st, out, total, sizes, _ = B.pack([r[1] for r in res], [B.crc32(c) for c in cs], [len(c) for c in cs], misalign=3)
    assert st == 0 and total == len(out) == sum(sizes)
    return out, sizes


def check_file(data, bs, out, sizes=None):
    """What every BGZF file of `data` cut at `bs` must satisfy, whoever wrote it."""
    cs = chunks_of(data, bs)
    assert gzip.decompress(out) == data
    assert out.endswith(B.EOF)
    refs = swc.index_blocks("bgzf", out)
    assert len(refs) == len(cs) + 1 and [r[2] for r in refs] == [len(c) for c in cs] + [0]
    pos = 0
    for k, (off, comp_len, _, _) in enumerate(refs):
        assert off == pos + 18 and out[pos:pos + 16] == B.HEADER
        size = struct.unpack_from("<H", out, pos + 16)[0] + 1
        assert size == 26 + comp_len and (sizes is None or sizes[k] == size)
        crc, isize = struct.unpack_from("<II", out, pos + size - 8)
        chunk = cs[k] if k < len(cs) else b""
        assert (crc, isize) == (zlib.crc32(chunk), len(chunk))
        assert zlib.decompress(out[off:off + comp_len], -15) == chunk
        pos += size
    assert pos == len(out) and (sizes is None or len(sizes) == len(refs))
    return refs


E2E = [(b"", 65280), (b"x", 65280), (corpus.p_text(200001, 5), 65280), (corpus.p_mix(200001, 6), 65280), (corpus.p_rand(200001, 7), 65280),
       (corpus.p_text(5000, 8), 37)]


@pytest.mark.parametrize("dynamic", [False, True])
@pytest.mark.parametrize("case", range(len(E2E)))
def test_end_to_end_on_the_emulation(case, dynamic):
    data, bs = E2E[case]
    out, sizes = emu_archive(data, bs, dynamic)
    refs = check_file(data, bs, out, sizes)
    assert len(out) <= len(data) + 31 * (len(refs) - 1) + 28
    if case == 4:   # random bytes: stored blocks, the member -- and BSIZE -- at their maximum
        assert sizes[:3] == [65311] * 3 and all(out[65311 * k + 18] == 1 for k in range(3))


# ---- ABI, host only -------------------------------------------------------------------------------------------------------------
def test_bound_and_block_size_rules():
    lib = _lib.load()
    for n in [0, 1, 65279, 65280, 65281, 200001, 5000, (1 << 32) + 5] + LENGTHS:
        for bs in (1, 37, 65279, 65280):
            assert lib.swc_bgzf_bound(n, bs) == n + 31 * -(-n // bs) + 28
        assert lib.swc_bgzf_bound(n, 0) == lib.swc_bgzf_bound(n, 65280)
    assert lib.swc_bgzf_workspace_bytes(200001, 65280) == B.plan(200001, 65280)["bytes"] + 16
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t(7)
    assert lib.swc_bgzf_archive(b"abc", 3, 65281, 0, C.byref(out), C.byref(n), None, None) == SWC_E_INVALID_ARGUMENT and n.value == 0
    lib.swc_free(out)
    meta = (C.c_uint64 * 4)()
    assert lib.swc_batch_bgzf_archive(C.addressof(meta), 3, 65281, 0, C.addressof(meta), 64, C.addressof(meta), None, None, 0, None) == SWC_E_INVALID_ARGUMENT
    with pytest.raises(swc.SWCError) as e:
        swc.GzipArchive.bgzf_archive(b"abc", block_size=65281)
    assert e.value.status == SWC_E_INVALID_ARGUMENT
    assert lib.swc_set_tuning(b"bgzf_round_members", 0) != 0 and lib.swc_set_tuning(b"bgzf_round_members", 16385) != 0
    assert lib.swc_set_tuning(b"bgzf_round_members", 16384) == 0


@pytest.mark.skipif(swc.device_available(), reason="GPU present: covered by the gpu tier")
def test_no_cpu_fallback_without_gpu():
    with pytest.raises(swc.DeviceError):
        swc.GzipArchive.bgzf_archive(corpus.p_text(1000, 1))
    with pytest.raises(swc.DeviceError):
        swc.GzipArchive.bgzf_archive(b"", dynamic=True, sizes=True)
