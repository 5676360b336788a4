"""A Deflate launch with linked units (csrc/inflate_sync.h, deflate_place.h, deflate_chain.h, lz_copy.h) on the host emulation: a
thin layer over _emu (tests/host_emu/emu_deflate_linked.cpp).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import struct

import _emu
from _emu import Job

lib = _emu.lib
set_order = _emu.set_order

GUARD = 16
JOINED, OPEN, LINKED = 1, 2, 4
RESOLVER, COPIER, BODY_ALONE = 0, 1, 2   # the arrangements of phase 2 (emu_deflate_linked.cpp)


def run_units(units, misalign=0, arrangement=COPIER, team=0, reversed_=False, crc=False):
    """One emulated launch.  units: list of dicts data / cap / aux.  Every job that is not joined starts a buffer of its own -- the sum
    of its run's capacities, `misalign` bytes past a 16-byte boundary, GUARD bytes of 0xA5 on both sides, 0xA5 throughout (_emu.Guarded).  Returns per
    job (status, out_len, in_consumed, aux, offset of `out` from its head's, bytes, reach, crc); asserts that every guard is intact
    and that nothing behind the last byte a run occupies was written."""
    n = len(units)
    jobs = (Job * n)()
    keep, bufs, head_of = [], {}, []
    for i, u in enumerate(units):
        ib = C.create_string_buffer(bytes(u["data"]), max(len(u["data"]), 1))
        keep.append(ib)
        jobs[i].in_ = C.addressof(ib)
        jobs[i].in_len = len(u["data"])
        jobs[i].out_cap = u["cap"]
        jobs[i].aux = u["aux"]
        jobs[i].status = 902
        if not (u["aux"] & JOINED) or i == 0:
            room = u["cap"]
            for v in units[i + 1:]:
                if not v["aux"] & JOINED:
                    break
                room += v["cap"]
            bufs[i] = _emu.Guarded(room, misalign, guard=GUARD)
            if not (u["aux"] & JOINED):
                jobs[i].out = bufs[i].addr
        head_of.append(max(k for k in bufs if k <= i))
    crcs = (C.c_uint32 * n)(*[0xA5A5A5A5] * n)
    reach = (C.c_uint32 * n)()
    lib.emu_deflate_linked(jobs, C.c_size_t(n), C.c_int(arrangement), C.c_int(team), C.c_int(1 if reversed_ else 0), crcs if crc else None, reach)
    res = []
    used = {h: 0 for h in bufs}
    for i in range(n):
        buf = bufs[head_of[i]]
        rel = (jobs[i].out or 0) - buf.addr
        k = min(jobs[i].out_len, jobs[i].out_cap)
        ok = jobs[i].out is not None and 0 <= rel and rel + k <= buf.n
        if ok:
            used[head_of[i]] = max(used[head_of[i]], rel + k)
        res.append((jobs[i].status, jobs[i].out_len, jobs[i].in_consumed, jobs[i].aux, rel if ok else None, buf.read(rel, rel + k) if ok else None,
                    reach[i], crcs[i] if crc else None))
    for h, buf in bufs.items():
        buf.check("the run of job %d" % h, used=used[h])
    return res


def case_file(cases):
    """The bytes of the file the stand-alone program reads.  cases: list of (units, expected) with expected per job (status, out_len, in_consumed,
    aux, bytes) as _deflate_linked_cases.expect gives it."""
    out = bytearray(struct.pack("<I", len(cases)))
    for units, exp in cases:
        out += struct.pack("<I", len(units))
        for u, (st, n, cons, aux, data) in zip(units, exp):
            pin = 0 if n is None else 1 if data is None else 2
            data = data if pin == 2 else b""
            out += struct.pack("<iI", u["aux"], len(u["data"])) + bytes(u["data"])
            out += struct.pack("<IiIIiII", u["cap"], st, pin, n if pin else 0, aux, cons if pin else 0, len(data)) + data
    return bytes(out)
