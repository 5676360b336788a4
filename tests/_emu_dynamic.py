"""ctypes binding of tests/host_emu/libswc_emu_deflate_dynamic.so -- the Deflate encoder's dynamic-block path and the shared
Huffman builder compiled for the host.  TEST INFRASTRUCTURE ONLY (see tests/host_emu/emu_deflate_dynamic.cpp)."""
import ctypes as C
import os
import subprocess

import _emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "host_emu")
SRC = os.path.join(_DIR, "emu_deflate_dynamic.cpp")
_LIB = os.path.join(_DIR, "libswc_emu_deflate_dynamic.so")
_CSRC = os.path.join(os.path.dirname(_HERE), "swcompression_amd", "csrc")
FLAGS = ["-std=c++17", "-DSWC_HOST_EMULATION", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-pthread"]


def build(force=False):
    srcs = [SRC] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")]
    if not force and os.path.exists(_LIB) and all(os.path.getmtime(_LIB) >= os.path.getmtime(s) for s in srcs):
        return
    subprocess.run(["g++", "-O2", "-g"] + FLAGS + ["-o", _LIB, SRC], check=True)


build()
lib = C.CDLL(_LIB)


def set_order(order):
    """Thread order of the emulated SIMT regions (csrc/simt.h): 0 forward, 1 reverse, 2 shuffled."""
    lib.emu_set_order(C.c_int(order))


def deflate_compress_dynamic(inputs, caps=None, aux=None):
    """Returns list of (status, stream, in_consumed, out_len); the guard bytes around every output are checked."""
    if caps is None:
        caps = [len(x) + len(x) // 8 + 32 for x in inputs]
    # _emu.run_batch (the job layout, the guard bytes) calls into _emu.lib by name: pointed at this library for the call
    saved = _emu.lib
    _emu.lib = lib
    try:
        return _emu.run_batch("emu_deflate_compress_dynamic", inputs, caps, aux=aux)
    finally:
        _emu.lib = saved


def huffman(weights, max_len):
    """The shared builder (csrc/huffman_wave.h): (lengths, canonical codes MSB first)."""
    n = len(weights)
    w = (C.c_uint32 * n)(*weights)
    ln = (C.c_uint32 * n)()
    cd = (C.c_uint32 * n)()
    lib.emu_huffman(w, C.c_uint32(n), C.c_uint32(max_len), ln, cd)
    return list(ln), list(cd)
