"""LZMA2 compression (csrc/lzma_comp.h) on the host emulation: tests/host_emu/emu_lzma_comp.cpp compiled into a small library of its
own, libswc_emu_lzma_comp.so, with _emu._compile's flags; rebuilt when its source, emu_util.h or a header of csrc is newer.  A thin
layer over _emu.run_batch.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import _emu

SRC = "emu_lzma_comp.cpp"
MAIN = "EMU_LZMA_COMP_MAIN"
_PATH = os.path.join(_emu._DIR, "libswc_emu_lzma_comp.so")

DICT_BYTE = 8        # what a reader of these runs needs: 64 KiB
CHUNK = 65536
SEGMENT = 1          # aux bit 0: the unit is a segment of a longer stream -- no end marker behind it


def _stale():
    deps = [os.path.join(_emu._DIR, SRC), os.path.join(_emu._DIR, "emu_util.h")]
    deps += [os.path.join(_emu._CSRC, f) for f in os.listdir(_emu._CSRC) if f.endswith(".h")]
    return not os.path.exists(_PATH) or os.path.getmtime(_PATH) < max(os.path.getmtime(d) for d in deps)


def build(force=False):
    if force or _stale():
        tmp = "%s.%d.tmp" % (_PATH, os.getpid())
        _emu._compile(tmp, SRC, ("-O2", "-g"), ("-fPIC", "-shared"))
        os.replace(tmp, _PATH)


build()
lib = C.CDLL(_PATH)
lib.emu_lzma2_compress_bound.argtypes = [C.c_uint64]
lib.emu_lzma2_compress_bound.restype = C.c_uint64


def set_order(order):
    """Thread order of the SIMT regions in this library: 0 forward, 1 reverse, 2 shuffled."""
    lib.emu_set_order(C.c_int(order))


def bound(n):
    """The largest run n bytes can turn into (lzma_comp.h: bound)."""
    return n + 3 * ((n + CHUNK - 1) // CHUNK) + 1


def compress(bufs, caps=None, aux=None, **place):
    """One run per buffer: returns list of (status, run bytes, in_consumed, out_len).  aux[i] & 1: unit i is a segment.  Always
    with exact=True: nothing may be written behind min(out_len, capacity)."""
    bufs = [bytes(b) for b in bufs]
    caps = caps or [bound(len(b)) for b in bufs]
    return _emu.run_batch("emu_lzma2_compress_jobs", bufs, caps, aux=aux, exact=True, lib=lib, **place)
