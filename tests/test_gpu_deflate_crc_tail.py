"""swc_batch_decompress_crc32_ws on the GPU: the Deflate copy kernel that ends with the CRC-32 of the stream it has written
(csrc/crc32_tail.h), its hand-over to the group kernel at 1 MiB, the ordered launch and the fall-back behind the workgroup
kernel -- against swc_batch_crc32 on the same job list, zlib.crc32 and the outputs of swc_batch_decompress_ws."""
import ctypes as C
import zlib

import numpy as np
import pytest

import _oracle as O
from swcompression_amd import _lib, corpus
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7C0DE
ROW = 2048
# the lengths of tests/test_crc_tail_emulation.py (every path of the tail) without its largest
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33]
for _size in (ROW, 2 * ROW, 3 * ROW, 4 * ROW, 5 * ROW, 8 * ROW, 12 * ROW, 13 * ROW, 16 * ROW):
    LENGTHS += [_size - 1, _size, _size + 1]
LENGTHS += [65535, 65536, 65537]


def _odd_cap(n):
    return n + 1 + (n % 2)


def _packed_batch(units, caps):
    """A DeviceBatch whose outputs lie back to back, capacity after capacity, instead of on 16-byte boundaries."""
    import torch
    b = DeviceBatch("deflate", units, caps)
    off = np.concatenate([[0], np.cumsum(np.array(caps, dtype=np.int64))[:-1]]).astype(np.int64)
    b._out_off = off
    b._jobs_host["out"] = (b.d_out.data_ptr() + off).astype(np.uint64)
    b.d_jobs.copy_(torch.from_numpy(b._jobs_host.view(np.uint8).copy()).to(b.device))
    return b


def _check(b, plains, expect_status=None):
    """Decodes `b` through swc_batch_decompress_ws and through the fused entry, and checks what the fused entry promises: no
    sentinel left, the CRCs of swc_batch_crc32 for every job, zlib's wherever the status is 0, the same
    bytes and the same job records as the plain launch.  Returns (status array, fused CRCs)."""
    import torch
    assert b._crc_buf is None   # (launch() below is the plain entry)
    b.wipe_results()
    b.launch(sync=True)
    plain_out = b.d_out.clone()
    plain_res = b.results().copy()
    b.wipe_results()
    crcs = torch.from_numpy(np.full(b.n, SENTINEL, dtype=np.uint32).view(np.int32).copy()).to(b.device)
    opts = _lib.SwcBatchOpts(b.device.index if b.device.index is not None else -1, torch.cuda.current_stream(b.device).cuda_stream, 1, 0)
    st = b.lib.swc_batch_decompress_crc32_ws(b.codec, b.d_jobs.data_ptr(), b.n, b.d_ws.data_ptr(), b.ws_bytes, crcs.data_ptr(), C.byref(opts))
    assert st == 0
    fused = crcs.cpu().numpy().view(np.uint32)
    res = b.results().copy()
    assert torch.equal(b.d_out, plain_out), "the fused launch wrote other bytes than swc_batch_decompress_ws"
    for f in ("status", "out_len", "in_consumed"):
        assert (res[f] == plain_res[f]).all(), f
    alone = b.crc32()   # the standalone kernels on the bytes in memory, the same job list
    bad = np.nonzero(fused != alone)[0]
    assert bad.size == 0, "jobs %s: fused %s, swc_batch_crc32 %s" % (bad[:8], fused[bad[:8]], alone[bad[:8]])
    ok = res["status"] == 0
    want = np.array([zlib.crc32(p) & 0xFFFFFFFF for p in plains], dtype=np.uint32)[b.unit_index]
    assert (fused[ok] == want[ok]).all()
    assert (fused != SENTINEL).all(), "jobs %s were left without a CRC" % np.nonzero(fused == SENTINEL)[0][:8]
    if expect_status is not None:
        for i, s in expect_status.items():
            assert (int(res["status"][i]) == s) if s >= 0 else (int(res["status"][i]) != 0), (i, int(res["status"][i]))
    return res["status"], fused


def test_batch_a_wave_kernel_on_a_small_batch():
    """About a hundred members in one launch that takes the wave kernel: every length at which the tail takes another path,
    outputs at all 16 residues, the hand-over to the group kernel, a capacity error and a corrupted stream."""
    lib = _lib.load()
    plains = [corpus.p_mix(n, 700 + i) if i % 2 else corpus.p_text(n, 700 + i) for i, n in enumerate(LENGTHS)]
    plains += [bytes(5000), b"\xff" * 4097, corpus.p_rand(3001, 9)]
    plains += [corpus.p_text((1 << 20) - 1, 31), corpus.p_mix(1 << 20, 32)]
    units = [corpus.deflate_raw(p) for p in plains]
    stored = corpus.p_rand(7001, 10)
    plains.append(stored)
    units.append(corpus.deflate_raw(stored, level=0))             # stored blocks only
    i_stored = len(units) - 1
    while len(units) < 98:
        p = corpus.p_text(1000 + 37 * len(units), 800 + len(units))
        plains.append(p)
        units.append(corpus.deflate_raw(p))
    caps = [_odd_cap(len(p)) for p in plains]
    short = corpus.p_text(30001, 33)                              # out_cap below its size
    plains.append(short[:20001])
    units.append(corpus.deflate_raw(short))
    caps.append(20001)
    i_short = len(units) - 1
    victim = corpus.p_text(40000, 34)                             # a corrupted stream: it breaks off in the middle of a block
    u = corpus.deflate_raw(victim)
    u = u[:len(u) // 2]
    assert O.deflate(u)[0] != 0 and len(O.deflate(u)[1]) > 10000   # (an error status behind output that was written)
    plains.append(victim)
    units.append(bytes(u))
    caps.append(_odd_cap(len(victim)))
    i_bad = len(units) - 1
    assert plains[LENGTHS.index(0)] == b"" and len(units) == 100
    try:
        assert lib.swc_set_tuning(b"lz_copier", -1) == 0
        b = _packed_batch(units, caps)
        assert set(int(x) % 16 for x in b._jobs_host["out"]) == set(range(16))
        status, fused = _check(b, plains, {i_stored: 0, i_short: 901, i_bad: -1, LENGTHS.index(0): 0})
        assert (np.delete(status, [i_short, i_bad]) == 0).all()
        # the capacity error: the CRC covers the out_cap bytes that exist
        assert int(fused[i_short]) == zlib.crc32(short[:20001]) & 0xFFFFFFFF
    finally:
        lib.swc_set_tuning(b"lz_copier", 1)


def test_batch_b_ordered_launch():
    """2,600 members of 1-4 KiB with the library's own choices: the wave kernel behind the ordering pass."""
    rng = np.random.Generator(np.random.PCG64(0x5C0DE + 801))
    base = [corpus.p_text(int(rng.integers(1024, 4097)), 900 + k) if k % 3 else corpus.p_mix(int(rng.integers(1024, 4097)), 900 + k)
            for k in range(130)]
    plains = [base[i % 130] for i in range(2600)]
    comp = [corpus.deflate_raw(p) for p in base]
    units = [comp[i % 130] for i in range(2600)]
    b = _packed_batch(units, [_odd_cap(len(p)) for p in plains])
    status, _ = _check(b, plains)
    assert (status == 0).all()


def test_batch_c_fallback_behind_the_workgroup_kernel():
    """64 members with the library's own choices: the workgroup kernel copies, the CRC kernels follow."""
    plains = [corpus.p_text(20000 + 911 * i, 1000 + i) if i % 2 else corpus.p_mix(3000 + 517 * i, 1000 + i) for i in range(62)]
    plains += [b"", corpus.p_rand(5, 3)]
    units = [corpus.deflate_raw(p) for p in plains]
    b = _packed_batch(units, [_odd_cap(len(p)) for p in plains])
    status, _ = _check(b, plains)
    assert (status == 0).all()


def test_device_batch_keeps_the_crcs_current():
    """launch(); crc32_async() leaves the CRCs of the launch in the buffer -- from the second launch on through the fused
    entry -- and after wipe_results() a crc32_async() without a launch computes what crc32() computes."""
    lib = _lib.load()
    plains = [corpus.p_text(3000 + 301 * i, 1100 + i) for i in range(40)]
    want = np.array([zlib.crc32(p) & 0xFFFFFFFF for p in plains], dtype=np.uint32)
    try:
        assert lib.swc_set_tuning(b"lz_copier", -1) == 0
        b = DeviceBatch("deflate", [corpus.deflate_raw(p) for p in plains], [len(p) for p in plains])
        for step in range(3):   # the first step: the standalone kernels; then the fused launch, and crc32_async() returns at once
            b.launch()
            b.crc32_async()
            assert b._crc_current == (step > 0)
            b.torch.cuda.synchronize()
            assert (b._crc_buf.cpu().numpy().view(np.uint32) == want).all(), step
            assert (b.crc32() == want).all()
        b.wipe_results()
        assert not b._crc_current
        b.crc32_async()
        b.torch.cuda.synchronize()
        got = b._crc_buf.cpu().numpy().view(np.uint32)
        assert (got == b.crc32()).all() and (got == 0).all()   # (every out_len is 0 after the wipe: the CRC-32 of nothing)
    finally:
        lib.swc_set_tuning(b"lz_copier", 1)
