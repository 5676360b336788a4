"""The BGZF writer's device code (csrc/bgzf_pack.h) on the host emulation: a thin layer over _emu (tests/host_emu/emu_bgzf.cpp).
TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import _emu

lib = _emu.lib
set_order = _emu.set_order
crc32 = _emu.crc32_wave   # the wave code the writer's CRC launch runs (crc32_wave.h)

GUARD = 16
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")   # the 16 bytes in front of BSIZE
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


lib.emu_bgzf_pack.restype = C.c_int


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
    ob = _emu.Guarded(cap, misalign, guard=GUARD)
    total = C.c_uint64(0)
    bad = C.c_uint64(0)
    sizes = (C.c_uint64 * (n + 1))()
    status = lib.emu_bgzf_pack(C.c_void_p(C.addressof(raw) + s0), C.c_uint64(stride), lens, st, cr, isz, C.c_uint64(n),
                               C.c_void_p(ob.addr), C.c_uint64(cap), C.c_int(1 if eof else 0), C.byref(total), sizes,
                               C.byref(bad))
    ob.check("pack")
    return status, ob.read(), total.value, [int(x) for x in sizes[:n + (1 if eof else 0)]], bad.value
