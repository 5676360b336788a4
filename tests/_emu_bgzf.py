"""ctypes binding of tests/host_emu/libswc_emu_bgzf.so -- the BGZF writer's device code (csrc/bgzf_pack.h) compiled for the host.
TEST INFRASTRUCTURE ONLY (see tests/host_emu/emu_bgzf.cpp).  The recipe is that of _emu.compile_lib."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "host_emu")
_SRC = os.path.join(_DIR, "emu_bgzf.cpp")
_LIB = os.path.join(_DIR, "libswc_emu_bgzf.so")
_CSRC = os.path.join(os.path.dirname(_HERE), "swcompression_amd", "csrc")

GUARD = 16
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")   # the 16 bytes in front of BSIZE
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def compile_lib(out, opt=("-O2", "-g")):
    subprocess.run(["g++"] + list(opt) + ["-std=c++17", "-DSWC_HOST_EMULATION", "-fPIC", "-shared",
                    "-Wno-unknown-pragmas", "-pthread", "-o", out, _SRC], check=True)


def build(force=False):
    srcs = [_SRC] + [os.path.join(_CSRC, f) for f in ("bgzf_pack.h", "crc32_wave.h", "simt.h", "swc_common.h")]
    if not force and os.path.exists(_LIB) and all(os.path.getmtime(_LIB) >= os.path.getmtime(s) for s in srcs):
        return
    compile_lib(_LIB)


build()
lib = C.CDLL(_LIB)
lib.emu_bgzf_crc32.argtypes = [C.c_char_p, C.c_size_t]
lib.emu_bgzf_crc32.restype = C.c_uint32
lib.emu_bgzf_pack.restype = C.c_int


def set_order(order):
    """Thread order of the emulated SIMT regions (csrc/simt.h): 0 forward, 1 reverse, 2 shuffled."""
    lib.emu_set_order(C.c_int(order))


def crc32(data):
    """CRC-32 by the wave code the writer's CRC launch runs (crc32_wave.h)."""
    data = bytes(data)
    return lib.emu_bgzf_crc32(data, len(data))


def plan(n_bytes, block_size):
    v = (C.c_uint64 * 9)()
    lib.emu_bgzf_plan(C.c_uint64(n_bytes), C.c_uint64(block_size), v)
    return dict(zip(("n", "stride", "cjobs", "kjobs", "crcs", "offs", "res", "slots", "bytes"), [int(x) for x in v]))


def pack(streams, crcs, isizes, dst_cap=None, misalign=0, eof=True, statuses=None):
    """Scan + pack of the members whose streams are `streams` (bytes each; laid out in 4-byte aligned slots as the compress launch
    leaves them).  The destination starts `misalign` bytes past a 16-byte boundary and has GUARD bytes of 0xA5 on either side of
    its dst_cap bytes (default: exactly what the file needs).  Returns (status, bytes written region [0, dst_cap), total,
    member sizes, index of the failing member); asserts that the guards are untouched."""
    n = len(streams)
    need = sum(26 + len(s) for s in streams) + (28 if eof else 0)
    cap = need if dst_cap is None else dst_cap
    stride = (max([len(s) for s in streams] + [0]) + 4 + 15) // 16 * 16
    raw = C.create_string_buffer(n * stride + 32)
    s0 = (-C.addressof(raw)) % 16
    C.memset(raw, 0xC3, len(raw))
    for i, s in enumerate(streams):
        C.memmove(C.addressof(raw) + s0 + i * stride, bytes(s), len(s))
    lens = (C.c_uint32 * max(n, 1))(*[len(s) for s in streams])
    st = (C.c_int32 * max(n, 1))(*(statuses or [0] * n))
    cr = (C.c_uint32 * max(n, 1))(*crcs)
    isz = (C.c_uint32 * max(n, 1))(*isizes)
    ob = C.create_string_buffer(cap + 2 * GUARD + 32)
    o0 = (-C.addressof(ob)) % 16 + GUARD + misalign
    C.memset(ob, 0xA5, len(ob))
    total = C.c_uint64(0)
    bad = C.c_uint64(0)
    sizes = (C.c_uint64 * (n + 1))()
    status = lib.emu_bgzf_pack(C.c_void_p(C.addressof(raw) + s0), C.c_uint64(stride), lens, st, cr, isz, C.c_uint64(n),
                               C.c_void_p(C.addressof(ob) + o0), C.c_uint64(cap), C.c_int(1 if eof else 0), C.byref(total), sizes,
                               C.byref(bad))
    out = ob.raw
    assert out[:o0] == b"\xA5" * o0 and out[o0 + cap:] == b"\xA5" * (len(out) - o0 - cap), "guard bytes overwritten"
    return status, out[o0:o0 + cap], total.value, [int(x) for x in sizes[:n + (1 if eof else 0)]], bad.value
