"""The scan for bzip2 marks (csrc/bzip2_scan.h) on the host emulation: tests/host_emu/emu_bzip2_marks.cpp compiled into a small
library of its own, libswc_emu_bzip2_marks.so, with _emu._compile's flags; rebuilt when its source, emu_util.h or a header of csrc
is newer.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

import _emu

SRC = "emu_bzip2_marks.cpp"
MAIN = "EMU_BZIP2_MARKS_MAIN"
_PATH = os.path.join(_emu._DIR, "libswc_emu_bzip2_marks.so")


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
lib.emu_bzip2_scan_tile_bytes.restype = C.c_uint32
lib.emu_bzip2_index.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
lib.emu_bzip2_index.restype = None
TILE = int(lib.emu_bzip2_scan_tile_bytes())
REF_BYTES = 32


def set_order(order):
    """Thread order of the SIMT regions, and wave order of the launches, in this library: 0 forward, 1 reverse, 2 shuffled."""
    lib.emu_set_order(C.c_int(order))


def refs_of(raw):
    """The refs in `raw` (32 bytes each) as tuples (offset, comp_len, uncomp_len, aux, flags)."""
    a = np.frombuffer(raw, dtype=np.dtype([("o", "<u8"), ("c", "<u8"), ("u", "<u8"), ("a", "<u4"), ("f", "<u4")]))
    return [tuple(int(x) for x in r) for r in a]


def index(data, cap, residue=0, room=None):
    """emu_bzip2_index of `data` placed `residue` bytes past a 16-byte boundary, the refs in a buffer of `room` refs (default: cap)
    that starts 8 bytes past one; both between guard bytes that are checked afterwards, the data for change too; *n pre-filled.
    Returns (n, the first min(n, cap) refs)."""
    data = bytes(data)
    src = _emu.Guarded(len(data), residue, guard=32, data=data)
    out = _emu.Guarded((cap if room is None else room) * REF_BYTES, 8, guard=64)
    n = C.c_uint64(0xEEEEEEEEEEEEEEEE)
    lib.emu_bzip2_index(C.c_void_p(src.addr), C.c_uint64(len(data)), C.c_void_p(out.addr), C.c_uint64(cap), C.byref(n))
    src.check("bzip2 index: the buffer")
    assert src.read() == data, "bzip2 index: the buffer changed"
    m = min(n.value, cap)
    out.check("bzip2 index: the refs", used=m * REF_BYTES)
    return n.value, refs_of(out.read(0, m * REF_BYTES))
