"""ctypes binding of tests/host_emu/libswc_emu_deflate_units.so -- a Deflate launch with joined and open units (csrc/inflate_sync.h,
deflate_place.h, lz_copy.h, lz_resolve.h) compiled for the host.  TEST INFRASTRUCTURE ONLY (see
tests/host_emu/emu_deflate_units.cpp).  The recipe is that of _emu.compile_lib."""
import ctypes as C
import os
import struct
import subprocess

from _emu import Job

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "host_emu")
_SRC = os.path.join(_DIR, "emu_deflate_units.cpp")
_LIB = os.path.join(_DIR, "libswc_emu_deflate_units.so")
_CSRC = os.path.join(os.path.dirname(_HERE), "swcompression_amd", "csrc")

GUARD = 16
JOINED, OPEN = 1, 2


def compile_lib(out, opt=("-O2", "-g")):
    subprocess.run(["g++"] + list(opt) + ["-std=c++17", "-DSWC_HOST_EMULATION", "-fPIC", "-shared",
                    "-Wno-unknown-pragmas", "-pthread", "-o", out, _SRC], check=True)


def compile_program(out, opt=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")):
    """The stand-alone program of emu_deflate_units.cpp (its own main), by default with the address and undefined-behaviour sanitizers."""
    subprocess.run(["g++"] + list(opt) + ["-std=c++17", "-DSWC_HOST_EMULATION", "-DEMU_DEFLATE_UNITS_MAIN",
                    "-Wno-unknown-pragmas", "-pthread", "-o", out, _SRC], check=True)


def build(force=False):
    srcs = [_SRC] + [os.path.join(_CSRC, f) for f in ("deflate_place.h", "inflate_sync.h", "inflate_lane.h", "lz_copy.h", "lz_resolve.h",
                                                       "simt.h", "swc_common.h")]
    if not force and os.path.exists(_LIB) and all(os.path.getmtime(_LIB) >= os.path.getmtime(s) for s in srcs):
        return
    compile_lib(_LIB)


build()
lib = C.CDLL(_LIB)


def set_order(order):
    """Thread order of the emulated SIMT regions (csrc/simt.h): 0 forward, 1 reverse, 2 shuffled."""
    lib.emu_set_order(C.c_int(order))


def place(sizes, caps, aux, base=0x10000, reversed_=False):
    """The placing scan alone: jobs with out_len = sizes[i], out_cap = caps[i], aux[i]; every job that is not joined gets
    out = base + 2^32 * i.  Returns per job (out, status, out_len); status 902 where the scan wrote none."""
    n = len(sizes)
    jobs = (Job * n)()
    for i in range(n):
        jobs[i].out_len, jobs[i].out_cap, jobs[i].aux, jobs[i].status = sizes[i], caps[i], aux[i], 902
        jobs[i].in_consumed = 7
        if not aux[i] & JOINED:
            jobs[i].out = base + (i << 32)
    lib.emu_deflate_place(jobs, C.c_size_t(n), C.c_int(1 if reversed_ else 0))
    return [(jobs[i].out or 0, jobs[i].status, jobs[i].out_len) for i in range(n)]


def run_units(units, misalign=0, copier=1, team=0, reversed_=False, head_gap=None):
    """One emulated launch.  units: list of dicts data / cap / aux.  Every job that is not joined starts a buffer of its own -- the sum
    of its run's capacities, `misalign` bytes past a 16-byte boundary, GUARD bytes of 0xA5 on both sides.  Returns per job (status,
    out_len, in_consumed, aux, offset of `out` from its head's, bytes); asserts that every guard is intact and that nothing behind
    the last byte a run produced was written."""
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
            buf = C.create_string_buffer(GUARD + 32 + room + GUARD)
            C.memset(buf, 0xA5, len(buf))
            o0 = (-C.addressof(buf)) % 16 + GUARD + misalign
            bufs[i] = (buf, o0, room)
            if not (u["aux"] & JOINED):
                jobs[i].out = C.addressof(buf) + o0
        head_of.append(max(k for k in bufs if k <= i))
    lib.emu_deflate_units(jobs, C.c_size_t(n), C.c_int(copier), C.c_int(team), C.c_int(1 if reversed_ else 0))
    res = []
    used = {h: 0 for h in bufs}
    for i in range(n):
        buf, o0, room = bufs[head_of[i]]
        rel = (jobs[i].out or 0) - (C.addressof(buf) + o0)
        k = min(jobs[i].out_len, jobs[i].out_cap)
        ok = jobs[i].out is not None and 0 <= rel and rel + k <= room
        if ok:
            used[head_of[i]] = max(used[head_of[i]], rel + k)
        res.append((jobs[i].status, jobs[i].out_len, jobs[i].in_consumed, jobs[i].aux, rel if ok else None, buf.raw[o0 + rel:o0 + rel + k] if ok else None))
    for h, (buf, o0, room) in bufs.items():
        raw = buf.raw
        assert raw[:o0] == b"\xA5" * o0, "bytes in front of the run of job %d overwritten" % h
        assert raw[o0 + used[h]:] == b"\xA5" * (len(raw) - o0 - used[h]), "bytes behind the run of job %d overwritten" % h
    return res


def write_cases(path, cases):
    """The file the stand-alone program reads.  cases: list of (units, expected) with expected per job (status, out_len, in_consumed,
    aux, bytes) as _deflate_units_cases.expect gives it: out_len None = a failed unit, of which only status and aux are compared."""
    out = bytearray(struct.pack("<I", len(cases)))
    for units, exp in cases:
        out += struct.pack("<I", len(units))
        for u, (st, n, cons, aux, data) in zip(units, exp):
            pinned = n is not None
            data = data if pinned else b""
            out += struct.pack("<iI", u["aux"], len(u["data"])) + bytes(u["data"])
            out += struct.pack("<IiIIiII", u["cap"], st, 1 if pinned else 0, n if pinned else 0, aux, cons if pinned else 0, len(data)) + data
    with open(path, "wb") as f:
        f.write(out)
