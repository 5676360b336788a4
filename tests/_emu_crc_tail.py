"""ctypes binding of tests/host_emu/libswc_emu_crc_tail.so -- the CRC tail of the Deflate copy kernel (csrc/crc32_tail.h) compiled
for the host.  TEST INFRASTRUCTURE ONLY (see tests/host_emu/emu_crc_tail.cpp).  The recipe is that of _emu.compile_lib."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "host_emu")
_SRC = os.path.join(_DIR, "emu_crc_tail.cpp")
_LIB = os.path.join(_DIR, "libswc_emu_crc_tail.so")
_CSRC = os.path.join(os.path.dirname(_HERE), "swcompression_amd", "csrc")


def compile_lib(out, opt=("-O2", "-g")):
    subprocess.run(["g++"] + list(opt) + ["-std=c++17", "-DSWC_HOST_EMULATION", "-fPIC", "-shared",
                    "-Wno-unknown-pragmas", "-pthread", "-o", out, _SRC], check=True)


def build(force=False):
    srcs = [_SRC] + [os.path.join(_CSRC, f) for f in ("crc32_tail.h", "crc32_wave.h", "lz_copy.h", "lz_resolve.h", "simt.h", "swc_common.h")]
    if not force and os.path.exists(_LIB) and all(os.path.getmtime(_LIB) >= os.path.getmtime(s) for s in srcs):
        return
    compile_lib(_LIB)


build()
lib = C.CDLL(_LIB)
lib.emu_crc_tail.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
lib.emu_crc_tail.restype = C.c_int


def set_order(order):
    """Thread order of the emulated SIMT regions (csrc/simt.h): 0 forward, 1 reverse, 2 shuffled."""
    lib.emu_set_order(C.c_int(order))


def crc32(data, residue=0):
    """CRC-32 of `data` by the tail, the data placed `residue` bytes past a 16-byte boundary with nothing readable but guard
    bytes of another value around it."""
    data = bytes(data)
    buf = C.create_string_buffer(len(data) + 64)
    C.memset(buf, 0xC3, len(buf))
    o = (-C.addressof(buf)) % 16 + 16 + residue
    C.memmove(C.addressof(buf) + o, data, len(data))
    crc = C.c_uint32(0)
    rc = lib.emu_crc_tail(C.c_void_p(C.addressof(buf) + o), len(data), C.byref(crc))
    assert rc == 0, "the tail wrote outside its 6,144 bytes of constants"
    return crc.value
