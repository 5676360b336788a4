"""Deflate.compress(data, dynamic=True) -- dynamic-Huffman blocks (BTYPE 10) built on the device (SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC,
csrc/deflate_comp.h).  An extension: the reference's encoder writes static or stored blocks only (Deflate+Compress.swift:22-213).

The contract: the same parse as the static path, one block per unit, the block dynamic only where that is strictly smaller
than the static one and stored where that is not larger than the better of the two -- so the stream is never larger than the
static path's, and where no block is dynamic its bytes ARE the static path's.  Every header keeps to the form zlib writes
(complete codes, 15 / 15 / 7 bits at most, each table run-length coded on its own).
CPU tier: the kernel source on the host emulation (tests/host_emu/emu.cpp, through tests/_emu_dynamic.py)."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import zlib

import pytest

import _emu as E
import _emu_dynamic as D
import _oracle as O
import test_deflate_compress as T
from swcompression_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ref_inline_vectors.json")))
GOLD_INPUTS = [s.encode("latin1") for s in GOLD["roundtrip_strings"]] + [bytes.fromhex(h) for h in GOLD["roundtrip_bytes"]]
EDGE = [b"", b"a", b"ab", b"abc", b"\0" * 70000, corpus.p_rand(70000, 61), corpus.p_rand(70000, 62), bytes(range(256))]


def inputs():
    return (T.payloads() + GOLD_INPUTS + EDGE
            + [corpus.p_text(65536, s) for s in (1, 2)] + [corpus.p_mix(65536, 3), corpus.p_rep(20000, 4), corpus.p_text(262144, 5)])


# ---------------------------------------------------------------------------------------------------------------- header checker
class Bits:
    def __init__(self, z, pos=0):
        self.z, self.pos = z, pos

    def get(self, n):
        v = 0
        for i in range(n):
            v |= ((self.z[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def kraft_complete(lens, limit):
    used = [n for n in lens if n]
    assert used and max(used) <= limit, (max(used), limit)
    assert sum(1 << (limit - n) for n in used) == 1 << limit, "Kraft sum is not exactly 1"


def canonical(lens):
    """{(length, code): symbol} of the canonical code of `lens` (RFC 1951 3.2.2)."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    tab = {}
    for s, n in enumerate(lens):
        if n:
            tab[(n, nxt[n])] = s
            nxt[n] += 1
    return tab


def check_dynamic_header(z, pos=0):
    """Parses the header of the dynamic block at bit `pos`: HLIT <= 286, HDIST <= 30, HCLEN >= 4, complete codes of at most
    15 / 15 / 7 bits, 16 never first in a table and no run across the two tables.  Returns (lit/len lengths, distance lengths)."""
    r = Bits(z, pos)
    r.get(1)
    assert r.get(2) == 2
    hlit, hdist, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    assert hlit <= 286 and hdist <= 30
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = r.get(3)
    kraft_complete(cl, 7)
    tab = canonical(cl)

    def sym():
        code, n = 0, 0
        while True:
            code, n = (code << 1) | r.get(1), n + 1
            assert n <= 7
            if (n, code) in tab:
                return tab[(n, code)]

    def table(count):
        out = []
        while len(out) < count:
            s = sym()
            if s < 16:
                out.append(s)
            elif s == 16:
                assert out, "16 first in a table"
                out += [out[-1]] * (3 + r.get(2))
            elif s == 17:
                out += [0] * (3 + r.get(3))
            else:
                out += [0] * (11 + r.get(7))
            assert len(out) <= count, "a run crosses from one table into the other"
        return out

    ll = table(hlit)
    dd = table(hdist)
    kraft_complete(ll, 15)
    kraft_complete(dd, 15)
    assert ll[256] != 0
    return ll, dd


def check(x, z, final=True):
    """Round trip under zlib and the reference's decoder restated (which must consume the whole stream), the block rule and, for
    a dynamic block, its header."""
    if final:
        assert zlib.decompress(z, -15) == x
        st, y, cons = O.deflate(z)
        assert (st, y, cons) == (0, x, len(z)), (st, cons, len(z))
    kind = (z[0] >> 1) & 3
    assert (z[0] & 1) == (1 if final else 0) and kind in (0, 1, 2)
    if kind == 0:
        assert len(z) == 5 + len(x) <= 65535
    if kind == 2:
        check_dynamic_header(z)
    return kind


def static(xs, aux=None):
    return E.deflate_compress(xs, aux=aux)


# ------------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("order", [0, 1, 2])
def test_round_trips_in_every_lane_order(order):
    xs = inputs()
    D.set_order(0)
    ref = [r[1] for r in D.deflate_compress_dynamic(xs)]
    D.set_order(order)
    try:
        res = D.deflate_compress_dynamic(xs)
    finally:
        D.set_order(0)
    for x, (st, z, cons, n), z0 in zip(xs, res, ref):
        assert st == 0 and n == len(z) and cons == len(x)
        check(x, z)
        assert z == z0, "the stream depends on the order of the lanes"


def test_never_larger_and_the_static_bytes_where_not_dynamic():
    xs = inputs()
    kinds = set()
    for x, (st, z, _, _), (st2, z2, _, _) in zip(xs, D.deflate_compress_dynamic(xs), static(xs)):
        assert st == st2 == 0
        assert len(z) <= len(z2), (len(x), len(z), len(z2))
        kind = (z[0] >> 1) & 3
        kinds.add(kind)
        if kind != 2:
            assert z == z2
        else:
            assert len(z) < len(z2)
    assert kinds == {0, 1, 2}


def test_ratio_against_the_static_block():
    for s in (11, 12, 13, 14, 15):
        x = corpus.p_text(65536, s)
        z, z2 = D.deflate_compress_dynamic([x])[0][1], static([x])[0][1]
        assert (z[0] >> 1) & 3 == 2 and len(z) <= 0.85 * len(z2), (s, len(z), len(z2))
    for s in (13, 14):
        x = corpus.p_mix(65536, s)
        z, z2 = D.deflate_compress_dynamic([x])[0][1], static([x])[0][1]
        assert len(z) <= 0.96 * len(z2), (s, len(z), len(z2))


def test_edge_cases_round_trip_with_complete_codes():
    """Empty and tiny inputs; one byte value (one literal and one distance symbol: fillers complete both codes); random data
    too long for a stored block (practically no match: distance fillers); every byte value once; the reference's vectors."""
    xs = EDGE + [b"\x2e\x20\x2e\x20\x2e\x20\x20", b"\x00" * 300] + GOLD_INPUTS
    for x, (st, z, cons, n) in zip(xs, D.deflate_compress_dynamic(xs)):
        assert st == 0 and n == len(z)
        check(x, z)
    z = D.deflate_compress_dynamic([b"\0" * 70000])[0][1]
    ll, dd = check_dynamic_header(z)
    assert sum(1 for v in dd if v) == 2                     # one distance symbol in use + one filler
    z = D.deflate_compress_dynamic([corpus.p_rand(70000, 61)])[0][1]
    assert (z[0] >> 1) & 3 == 2                             # too long to store


def test_builder_on_its_own():
    def kraft(lens, limit):
        assert max(lens) <= limit and sum(1 << (limit - n) for n in lens) == 1 << limit

    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    lens, codes = D.huffman(fib, 15)
    kraft(lens, 15)
    assert max(lens) == 15                                  # (29 without the limit)
    lens, codes = D.huffman([5, 9], 15)
    assert lens == [1, 1] and codes == [0, 1]
    lens, codes = D.huffman([7] * 286, 15)
    kraft(lens, 15)
    assert sorted(set(lens)) == [8, 9]
    lens, codes = D.huffman([1 << k for k in range(19)], 7)
    kraft(lens, 7)
    # canonical: in order of (length, symbol)
    tab = canonical(lens)
    assert all(codes[s] == c for (n, c), s in tab.items())


def test_capacity_reports_the_size_and_writes_nothing_past_it():
    for x in (corpus.p_text(20000, 41), corpus.p_rand(3000, 42), corpus.p_text(400, 43)):
        full = D.deflate_compress_dynamic([x])[0]
        size = len(full[1])
        st, z, cons, n = D.deflate_compress_dynamic([x], caps=[size - 7])[0]      # (_emu.run_batch checks the guard bytes)
        assert st == 901 and n == size


def test_segments_of_a_longer_stream_join_into_one():
    """job.aux bit 0 with the dynamic codec: every segment is its own block with its own tables; a non-final Huffman block is
    followed by an empty stored block, so the segments one behind the other are one stream."""
    import random
    rnd = random.Random(3)
    segs = [corpus.p_text(70000, 1), corpus.p_rand(3000, 2), b"", b"a", b"ab", corpus.p_text(333, 3), corpus.p_rep(5000, 4), corpus.p_rand(70000, 5)]
    segs += [corpus.p_text(rnd.randint(1, 400), 10 + i) for i in range(24)] + [corpus.p_text(4097, 6), corpus.p_mix(50000, 7)]
    aux = [1] * (len(segs) - 1) + [0]
    res = D.deflate_compress_dynamic(segs, aux=aux)
    res2 = static(segs, aux=aux)
    stream = b""
    dyn = 0
    for (st, z, _, zl), s, (_, z2, _, _) in zip(res[:-1], segs[:-1], res2[:-1]):
        assert st == 0 and zl == len(z) and len(z) <= len(z2)
        kind = check(s, z, final=False)
        if kind in (1, 2):
            assert z[-4:] == b"\x00\x00\xff\xff"
        dyn += kind == 2
        stream += z
    assert dyn >= 3
    assert res[-1][0] == 0 and res[-1][1][0] & 1 == 1
    stream += res[-1][1]
    plain = b"".join(segs)
    assert zlib.decompress(stream, -15) == plain
    st, out, used = O.deflate(stream)
    assert (st, out) == (0, plain) and used == len(stream)


ASAN_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import _emu_dynamic as D
from swcompression_amd import corpus
D.lib = ctypes.CDLL(sys.argv[2])
xs = [b"", b"a", b"\0" * 70000, corpus.p_rand(70000, 1), corpus.p_text(65536, 2), corpus.p_mix(30000, 3), bytes(range(256))]
for order in (0, 1, 2):
    D.set_order(order)
    for (st, z, _, n), x in zip(D.deflate_compress_dynamic(xs), xs):
        assert st == 0 and n == len(z), (st, n, len(z))
    D.deflate_compress_dynamic(xs[2:5], caps=[10, 100, 1000])
    D.deflate_compress_dynamic(xs, aux=[1] * len(xs))
D.huffman([1] * 288, 15)
print("asan-clean")
"""


def test_dynamic_emulation_is_asan_clean(tmp_path):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not asan or not os.path.isabs(asan) or shutil.which("g++") is None:
        pytest.skip("no AddressSanitizer runtime")
    lib = str(tmp_path / "libswc_emu_asan.so")
    E.compile_lib(lib, opt=("-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer"))
    child = tmp_path / "child.py"
    child.write_text(ASAN_CHILD)
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0",
               PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), os.environ.get("PYTHONPATH", "")]))
    p = subprocess.run([sys.executable, str(child), HERE, lib], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "asan-clean" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])


def test_no_device_the_new_entry_points_report_it():
    import swcompression_amd as swc
    from swcompression_amd import _lib
    if swc.device_available():
        pytest.skip("GPU present: covered by the gpu tier")
    lib = _lib.load()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t()
    x = b"abcabcabc" * 10
    assert lib.swc_deflate_compress_dynamic(x, len(x), C.byref(out), C.byref(n)) == 902
    assert lib.swc_zlib_archive_dynamic(x, len(x), C.byref(out), C.byref(n)) == 902
    assert lib.swc_gzip_archive_dynamic(x, len(x), None, 0, None, 0, 0, 0, 255, 0, 0, None, 0, C.byref(out), C.byref(n)) == 902
    with pytest.raises(swc.DeviceError):
        swc.Deflate.compress(x, dynamic=True)
    with pytest.raises(swc.DeviceError):
        swc.ZlibArchive.archive(x, dynamic=True)
    with pytest.raises(swc.DeviceError):
        swc.GzipArchive.archive(x, dynamic=True)
