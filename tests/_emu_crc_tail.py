"""The CRC tail of the Deflate copy kernel (csrc/crc32_tail.h) on the host emulation: a thin layer over _emu
(tests/host_emu/emu_crc_tail.cpp).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import _emu

lib = _emu.lib
set_order = _emu.set_order
lib.emu_crc_tail.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
lib.emu_crc_tail.restype = C.c_int


def crc32(data, residue=0):
    """CRC-32 of `data` by the tail, the data placed `residue` bytes past a 16-byte boundary with nothing readable but guard
    bytes of another value around it."""
    buf = _emu.Guarded(len(data), residue, fill=0xC3, data=data)
    crc = C.c_uint32(0)
    rc = lib.emu_crc_tail(C.c_void_p(buf.addr), buf.n, C.byref(crc))
    assert rc == 0, "the tail wrote outside its 6,144 bytes of constants"
    buf.check("crc tail")
    return crc.value
