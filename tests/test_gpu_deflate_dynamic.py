"""GPU tier of Deflate.compress(data, dynamic=True) (SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC): the single-shot calls and the archive
writers against zlib / gzip, the reference's decoder restated and the engine's own decoder, byte for byte against the host
emulation of the same kernel source; the segmented path; a batch of 4,096 units decoded again on the device."""
import gzip
import zlib

import pytest

import _emu as E
import _emu_dynamic as D
import _oracle as O
import test_deflate_compress_dynamic as T
from swcompression_amd import corpus

pytestmark = pytest.mark.gpu


def single_inputs():
    return [corpus.p_text(65536, 11), corpus.p_text(200000, 12), corpus.p_mix(65536, 13), corpus.p_mix(300000, 14)] + T.EDGE + T.GOLD_INPUTS


def test_single_shot_calls_decode_and_equal_the_emulation():
    import swcompression_amd as swc
    xs = single_inputs()
    emu = D.deflate_compress_dynamic(xs)
    for x, (st, ze, _, _) in zip(xs, emu):
        assert st == 0
        z = swc.Deflate.compress(x, dynamic=True)
        assert z == ze
        T.check(x, z)
        assert swc.Deflate.decompress(z) == x
        a = swc.ZlibArchive.archive(x, dynamic=True)
        assert a[:2] == bytes([120, 218]) and a[2:-4] == ze
        assert zlib.decompress(a) == x and swc.ZlibArchive.unarchive(a) == x and O.zlib_unarchive(a)[:2] == (0, x)
        g = swc.GzipArchive.archive(x, dynamic=True)
        assert g[:10] == swc.GzipArchive.archive(b"")[:10] and g[10:-8] == ze
        assert gzip.decompress(g) == x and O.gzip_unarchive(g) == (0, x) and swc.GzipArchive.unarchive(g) == x
    g = swc.GzipArchive.archive(xs[0], file_name="a.txt", write_header_crc=True, dynamic=True)
    assert gzip.decompress(g) == xs[0] and g[:10] == swc.GzipArchive.archive(xs[0], file_name="a.txt", write_header_crc=True)[:10]


def test_segmented_buffer_is_one_stream_no_larger_than_static():
    import swcompression_amd as swc
    x = corpus.p_text(2 << 20, 21) + corpus.p_mix(1 << 20, 22) + corpus.p_rand(17, 23)
    assert len(x) == 3 * (1 << 20) + 17
    z = swc.Deflate.compress(x, dynamic=True)
    assert z[0] & 1 == 0 and (z[0] >> 1) & 3 == 2
    assert zlib.decompress(z, -15) == x
    st, out, used = O.deflate(z)
    assert (st, out) == (0, x) and used == len(z)
    assert swc.Deflate.decompress(z) == x
    assert len(z) <= len(swc.Deflate.compress(x))


def test_batch_of_4096_decodes_on_the_device():
    import numpy as np
    from swcompression_amd.batch import DeviceBatch
    plains = [corpus.p_text(65536, 900 + i) if i % 4 else corpus.p_mix(65536, 900 + i) for i in range(4096)]
    caps = [65536 + 65536 // 8 + 32] * len(plains)
    enc = DeviceBatch("deflate_compress_dynamic", plains, caps)
    enc.launch(sync=True)
    r = enc.results()
    assert (r["status"] == 0).all()
    streams = [enc.output(i, int(r["out_len"][i])) for i in range(len(plains))]
    for i in (0, 1, 2, 3, 2047, 4095):
        T.check(plains[i], streams[i])
    dec = DeviceBatch("deflate", streams, [65536] * len(plains))
    dec.launch(sync=True)
    d = dec.results()
    assert (d["status"] == 0).all() and (d["out_len"] == 65536).all()
    want = np.array([zlib.crc32(p) & 0xFFFFFFFF for p in plains], dtype=np.uint32)
    assert (dec.crc32() == want).all()
    st8 = DeviceBatch("deflate_compress", plains, caps)
    st8.launch(sync=True)
    r8 = st8.results()
    assert (r8["status"] == 0).all()
    total, total8 = int(r["out_len"].sum()), int(r8["out_len"].sum())
    assert total <= 0.90 * total8, (total, total8)


def test_default_is_unchanged():
    import swcompression_amd as swc
    from swcompression_amd.batch import DeviceBatch
    xs = [corpus.p_text(65536, 31), corpus.p_mix(20000, 32), b"", b"abc", corpus.p_rand(70000, 33)]
    enc = DeviceBatch("deflate_compress", xs, [len(x) + len(x) // 8 + 32 for x in xs])
    enc.launch(sync=True)
    r = enc.results()
    for i, x in enumerate(xs):
        z = swc.Deflate.compress(x)
        assert z == swc.Deflate.compress(x, dynamic=False)
        assert int(r["status"][i]) == 0 and z == enc.output(i, int(r["out_len"][i]))
        assert z == E.deflate_compress([x])[0][1]
