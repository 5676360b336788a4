"""The LZ4 path for jobs with history (csrc/lz4_wave.h, lz_copy.h, lz4_chain.h) on the host emulation: a thin layer over _emu
(tests/host_emu/emu_lz4_linked.cpp).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import struct

import _emu
from _emu import Job

lib = _emu.lib
set_order = _emu.set_order

GUARD = 16


def run_chains(chains, misalign=0, copier=1, exact=False):
    """Chains (tests/_lz4_linked_cases.py) as ONE job list through one emulated launch -- copier: 1 = of kCopierMin jobs and more (one
    record-mode parse, the chain copier over all jobs), 0 = a smaller one (the four-kernel split).  Every chain has a buffer of its
    own -- the prefix, then the sum of the capacities -- that starts `misalign` bytes past a 16-byte boundary (the head's `out` where
    the prefix is empty) and has GUARD bytes of 0xA5 on both sides.  Returns per chain the list, per job, of (status, out_len,
    in_consumed, offset of `out` from the head's, bytes); asserts that the guards and the prefixes are untouched -- with `exact`, also
    every byte of the buffer behind the last one a job of the chain reports."""
    n = sum(len(ch["jobs"]) for ch in chains)
    jobs = (Job * n)()
    keep, bufs, i = [], [], 0
    for ch in chains:
        prefix = ch["prefix"]
        buf = _emu.Guarded(len(prefix) + sum(j["cap"] for j in ch["jobs"]), misalign, guard=GUARD, data=prefix)
        bufs.append(buf)
        jobs[i].out = buf.addr + len(prefix)
        for k, j in enumerate(ch["jobs"]):
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
            if k == 0 and prefix:
                jobs[i].dict = buf.addr
                jobs[i].dict_len = len(prefix)
            i += 1
    lib.emu_lz4_linked(jobs, C.c_size_t(n), C.c_int(copier))
    out, i = [], 0
    for ch, buf in zip(chains, bufs):
        prefix = ch["prefix"]
        room, out0 = buf.n - len(prefix), buf.addr + len(prefix)
        assert buf.read(0, len(prefix)) == prefix, "prefix overwritten"
        res, end = [], len(prefix)
        for _ in ch["jobs"]:
            rel = (jobs[i].out or 0) - out0
            k = min(jobs[i].out_len, jobs[i].out_cap)
            at = len(prefix) + rel
            if 0 <= rel <= room:
                end = max(end, min(at + k, buf.n))
            res.append((jobs[i].status, jobs[i].out_len, jobs[i].in_consumed, rel, buf.read(at, min(at + k, buf.n)) if 0 <= rel <= room else None))
            i += 1
        buf.check(ch["name"], used=end if exact else None)
        out.append(res)
    return out


def run_chain(ch, misalign=0, copier=1):
    """One chain alone in a launch (run_chains)."""
    return run_chains([ch], misalign, copier)[0]


def jobs_taken(reset=True):
    """How many jobs the decoding paths of the launches since the last reset took -- the lane decoder, the byte-cell resolver, the
    waves of the chain copier -- added up (csrc/lz4_wave.h: g_lz4_stats[5])."""
    st = (C.c_uint64 * 8)()
    lib.emu_lz4_stats(st, C.c_int(1 if reset else 0))
    return st[5]


def case_file(cases, expected):
    """The bytes of the file the stand-alone program reads: `cases` with what the oracle says (expected(case) -> per job (status, bytes, out_len))."""
    out = bytearray(struct.pack("<I", len(cases)))
    for ch in cases:
        exp = expected(ch)
        out += struct.pack("<I", len(ch["prefix"])) + ch["prefix"] + struct.pack("<I", len(ch["jobs"]))
        for j, (st, _, n) in zip(ch["jobs"], exp):
            assert j["dict"] is None
            out += struct.pack("<iI", j["aux"], len(j["data"])) + j["data"] + struct.pack("<IiI", j["cap"], st, n)
        want = b"".join(e[1] for e in exp)
        out += struct.pack("<I", len(want)) + want
    return bytes(out)
