"""The Deflate encoder's dynamic-block path and the shared Huffman builder on the host emulation: a thin layer over _emu
(tests/host_emu/emu.cpp).  TEST INFRASTRUCTURE ONLY.  `lib` is the handle the calls go to: the ASAN child points it at its build."""
import ctypes as C

import _emu

build = _emu.build
lib = _emu.lib


def set_order(order):
    """Thread order of the emulated SIMT regions (csrc/simt.h): 0 forward, 1 reverse, 2 shuffled."""
    lib.emu_set_order(C.c_int(order))


def deflate_compress_dynamic(inputs, caps=None, aux=None, **place):
    """Returns list of (status, stream, in_consumed, out_len); the guard bytes around every output are checked."""
    if caps is None:
        caps = [len(x) + len(x) // 8 + 32 for x in inputs]
    return _emu.run_batch("emu_deflate_compress_dynamic", inputs, caps, aux=aux, lib=lib, **place)


def huffman(weights, max_len):
    """The shared builder (csrc/huffman_wave.h): (lengths, canonical codes MSB first)."""
    n = len(weights)
    w = (C.c_uint32 * n)(*weights)
    ln = (C.c_uint32 * n)()
    cd = (C.c_uint32 * n)()
    lib.emu_huffman(w, C.c_uint32(n), C.c_uint32(max_len), ln, cd)
    return list(ln), list(cd)
