"""ctypes binding of tests/host_emu/libswc_emu_lz4_linked.so -- the LZ4 path for jobs with history (csrc/lz4_wave.h, lz_copy.h,
lz4_chain.h) compiled for the host.  TEST INFRASTRUCTURE ONLY (see tests/host_emu/emu_lz4_linked.cpp).  The recipe is that of
_emu.compile_lib."""
import ctypes as C
import os
import struct
import subprocess

from _emu import Job

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "host_emu")
_SRC = os.path.join(_DIR, "emu_lz4_linked.cpp")
_LIB = os.path.join(_DIR, "libswc_emu_lz4_linked.so")
_CSRC = os.path.join(os.path.dirname(_HERE), "swcompression_amd", "csrc")

GUARD = 16


def compile_lib(out, opt=("-O2", "-g")):
    subprocess.run(["g++"] + list(opt) + ["-std=c++17", "-DSWC_HOST_EMULATION", "-fPIC", "-shared",
                    "-Wno-unknown-pragmas", "-pthread", "-o", out, _SRC], check=True)


def compile_program(out, opt=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")):
    """The stand-alone program of emu_lz4_linked.cpp (its own main), by default with the address and undefined-behaviour sanitizers."""
    subprocess.run(["g++"] + list(opt) + ["-std=c++17", "-DSWC_HOST_EMULATION", "-DEMU_LZ4_LINKED_MAIN",
                    "-Wno-unknown-pragmas", "-pthread", "-o", out, _SRC], check=True)


def build(force=False):
    srcs = [_SRC] + [os.path.join(_CSRC, f) for f in ("lz4_chain.h", "lz4_wave.h", "lz4_lane.h", "lz_copy.h", "lz_resolve.h", "simt.h",
                                                       "swc_common.h")]
    if not force and os.path.exists(_LIB) and all(os.path.getmtime(_LIB) >= os.path.getmtime(s) for s in srcs):
        return
    compile_lib(_LIB)


build()
lib = C.CDLL(_LIB)


def set_order(order):
    """Thread order of the emulated SIMT regions (csrc/simt.h): 0 forward, 1 reverse, 2 shuffled."""
    lib.emu_set_order(C.c_int(order))


def run_chain(ch, misalign=0):
    """One chain (tests/_lz4_linked_cases.py) through one emulated launch.  The chain's buffer -- the prefix, then the sum of the
    capacities -- starts `misalign` bytes past a 16-byte boundary (the head's `out` where the prefix is empty) and has GUARD bytes
    of 0xA5 on both sides.  Returns per job (status, out_len, in_consumed, offset of `out` from the head's, bytes); asserts that
    the guards and the prefix are untouched."""
    jobs_in = ch["jobs"]
    n = len(jobs_in)
    prefix = ch["prefix"]
    room = sum(j["cap"] for j in jobs_in)
    buf = C.create_string_buffer(GUARD + 16 + 16 + len(prefix) + room + GUARD)
    C.memset(buf, 0xA5, len(buf))
    p0 = (-C.addressof(buf)) % 16 + GUARD + misalign     # where the prefix starts
    o0 = p0 + len(prefix)
    C.memmove(C.addressof(buf) + p0, prefix, len(prefix))
    jobs = (Job * n)()
    keep = []
    for i, j in enumerate(jobs_in):
        ib = C.create_string_buffer(j["data"], max(len(j["data"]), 1))
        keep.append(ib)
        jobs[i].in_ = C.addressof(ib)
        jobs[i].in_len = len(j["data"])
        jobs[i].out_cap = j["cap"]
        jobs[i].aux = j["aux"]
        jobs[i].status = 902
        if j["dict"] is not None:
            db = C.create_string_buffer(j["dict"], max(len(j["dict"]), 1))
            keep.append(db)
            jobs[i].dict = C.addressof(db)
            jobs[i].dict_len = len(j["dict"])
    jobs[0].out = C.addressof(buf) + o0
    if prefix:
        jobs[0].dict = C.addressof(buf) + p0
        jobs[0].dict_len = len(prefix)
    lib.emu_lz4_linked(jobs, C.c_size_t(n))
    raw = buf.raw
    assert raw[:p0] == b"\xA5" * p0 and raw[o0 + room:] == b"\xA5" * (len(raw) - o0 - room), "guard bytes overwritten (%s)" % ch["name"]
    assert raw[p0:o0] == prefix, "prefix overwritten"
    res = []
    for i in range(n):
        rel = (jobs[i].out or 0) - (C.addressof(buf) + o0)
        k = min(jobs[i].out_len, jobs[i].out_cap)
        res.append((jobs[i].status, jobs[i].out_len, jobs[i].in_consumed, rel, raw[o0 + rel:o0 + rel + k] if 0 <= rel <= room else None))
    return res


def write_cases(path, cases, expected):
    """The file the stand-alone program reads: `cases` with what the oracle says (expected(case) -> per job (status, bytes, out_len))."""
    out = bytearray(struct.pack("<I", len(cases)))
    for ch in cases:
        exp = expected(ch)
        out += struct.pack("<I", len(ch["prefix"])) + ch["prefix"] + struct.pack("<I", len(ch["jobs"]))
        for j, (st, _, n) in zip(ch["jobs"], exp):
            assert j["dict"] is None
            out += struct.pack("<iI", j["aux"], len(j["data"])) + j["data"] + struct.pack("<IiI", j["cap"], st, n)
        want = b"".join(e[1] for e in exp)
        out += struct.pack("<I", len(want)) + want
    with open(path, "wb") as f:
        f.write(out)
