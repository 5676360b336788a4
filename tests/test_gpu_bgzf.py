"""GPU tier of the BGZF writer (swc_bgzf_archive / swc_batch_bgzf_archive): round trips through gzip, the host indexer and the
engine's own one-launch decoder; byte for byte against the single-shot encoder and a packer written here at every border
alignment; the device-resident entry through torch tensors with its capacity and workspace rules; the rounds of the host entry."""
import struct
import zlib

import numpy as np
import pytest

import _emu_bgzf as B
import test_bgzf_pack_emulation as T
import swcompression_amd as swc
from swcompression_amd import _lib, batch, corpus

pytestmark = pytest.mark.gpu

SWC_E_CAPACITY, SWC_E_NEED_WORKSPACE = 901, 904
TEXT = corpus.p_text(3 * 65280 + 17, 31)
ROUND_TRIP = [TEXT[:n] for n in (0, 1, 65279, 65280, 65281, 3 * 65280 + 17)] + [corpus.p_mix(1 << 20, 32), corpus.p_rand(300000, 33)]


@pytest.mark.parametrize("dynamic", [False, True])
def test_round_trip_through_the_host_entry(dynamic):
    for data in ROUND_TRIP:
        out, sizes = swc.GzipArchive.bgzf_archive(data, dynamic=dynamic, sizes=True)
        assert sum(sizes) == len(out) <= _lib.load().swc_bgzf_bound(len(data), 65280)
        refs = T.check_file(data, 65280, out, sizes)
        parts = swc.GzipArchive.multi_unarchive(out)
        assert len(parts) == len(refs) and parts[-1] == b"" and b"".join(parts) == data
        assert swc.GzipArchive.bgzf_archive(data, dynamic=dynamic) == out
    rand = swc.GzipArchive.bgzf_archive(ROUND_TRIP[-1], dynamic=dynamic, sizes=True)[1]
    assert rand[:4] == [65311] * 4


def expected_file(data, bs, dynamic):
    """The file built from the shipped single-shot encoder and the packer of the CPU tier."""
    return b"".join(T.member(swc.Deflate.compress(c, dynamic=dynamic), zlib.crc32(c), len(c)) for c in T.chunks_of(data, bs)) + B.EOF


# Every block size moves the borders by another member size: 1..40 make members of 29 to about 60 bytes -- all head, or one or two
# interior chunks -- at every alignment; 255-257 and 4,093 run the interior loop below and above one step of the wave.
BLOCK_SIZES = list(range(1, 41)) + [255, 256, 257, 4093]


@pytest.mark.parametrize("dynamic", [False, True])
def test_byte_exact_against_the_single_shot_encoder(dynamic):
    text, mix = corpus.p_text(5000, 41), corpus.p_mix(70000, 42)
    for bs, data in [(bs, text) for bs in BLOCK_SIZES] + [(257, mix)]:
        out = swc.GzipArchive.bgzf_archive(data, block_size=bs, dynamic=dynamic)
        assert out == expected_file(data, bs, dynamic), "block_size %d" % bs


def test_device_resident_entry_through_torch_tensors():
    import torch
    bs, n = 16384, 4096
    distinct = [corpus.p_text(bs, 500 + k) if k % 4 else corpus.p_mix(bs, 500 + k) for k in range(512)]
    data = b"".join(distinct) * (n // 512)
    dev = torch.device("cuda:0")
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    lib = _lib.load()
    cap = lib.swc_bgzf_bound(len(data), bs)
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.empty(batch.bgzf_workspace_bytes(len(data), bs), dtype=torch.uint8, device=dev)
    st, total, sizes = batch.bgzf_archive(src, dst, block_size=bs, workspace=ws)
    assert st == 0 and 28 * (n + 1) < total < len(data)
    host = dst.cpu().numpy().tobytes()
    out = host[:total]
    assert host[total:] == b"\xA5" * (cap - total)
    # a host parse of the file: member sizes from BSIZE
    pos, parsed = 0, []
    while pos < total:
        assert out[pos:pos + 16] == B.HEADER
        parsed.append(struct.unpack_from("<H", out, pos + 16)[0] + 1)
        pos += parsed[-1]
    assert pos == total and len(parsed) == n + 1 and parsed == [int(x) for x in sizes] and out.endswith(B.EOF)
    # the 512 distinct chunks repeat: so do their members
    assert parsed[:512] * (n // 512) == parsed[:n]
    parts = swc.GzipArchive.multi_unarchive(out)
    assert len(parts) == n + 1 and b"".join(parts) == data
    # one byte short: the needed length, nothing written
    dst.fill_(0x5A)
    st2, total2, _ = batch.bgzf_archive(src, dst, block_size=bs, workspace=ws, dst_cap=total - 1)
    assert (st2, total2) == (SWC_E_CAPACITY, total)
    assert bool((dst == 0x5A).all())
    # half the workspace
    st3, _, _ = batch.bgzf_archive(src, dst, block_size=bs, workspace=ws[:ws.numel() // 2])
    assert st3 == SWC_E_NEED_WORKSPACE and bool((dst == 0x5A).all())
    # the same file with dynamic blocks decodes too and is smaller
    st4, total4, _ = batch.bgzf_archive(src, dst, block_size=bs, dynamic=True, workspace=ws)
    assert st4 == 0 and total4 < total
    assert b"".join(swc.GzipArchive.multi_unarchive(dst[:total4].cpu().numpy().tobytes())) == data


def test_rounds_of_the_host_entry():
    lib = _lib.load()
    data = corpus.p_text(19 * 4000 + 123, 61)
    whole, whole_sizes = swc.GzipArchive.bgzf_archive(data, block_size=4000, sizes=True)
    assert len(whole_sizes) == 21
    try:
        assert lib.swc_set_tuning(b"bgzf_round_members", 8) == 0
        for dynamic in (False, True):
            ref = whole if not dynamic else None
            out, sizes = swc.GzipArchive.bgzf_archive(data, block_size=4000, dynamic=dynamic, sizes=True)
            if ref is not None:
                assert out == ref and sizes == whole_sizes
            assert out.count(B.EOF) == 1 and out.endswith(B.EOF) and len(sizes) == 21
            T.check_file(data, 4000, out, sizes)
        # a round boundary at the very end: 16 members are two full rounds, the end-of-file member comes with the second
        out = swc.GzipArchive.bgzf_archive(data[:16 * 4000], block_size=4000)
        assert out.count(B.EOF) == 1 and len(T.check_file(data[:16 * 4000], 4000, out)) == 17
    finally:
        assert lib.swc_set_tuning(b"bgzf_round_members", 16384) == 0
    assert swc.GzipArchive.bgzf_archive(data, block_size=4000) == whole
