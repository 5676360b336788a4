"""SHA-256 by one lane per job (csrc/sha256_lane.h, the body of csrc/job_kernels.h) on the host emulation: a thin layer over
_emu (tests/host_emu/emu_sha256.cpp).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import _emu
from _emu import Job
from _sha256_cases import LENGTHS, message, mix  # noqa: F401

lib = _emu.lib
lib.emu_sha256_jobs.argtypes = [C.POINTER(Job), C.c_size_t, C.c_void_p]
lib.emu_sha256_jobs.restype = None


def run(jobs, residue=0, digest_residue=1):
    """One emulated launch.  Every job's bytes lie in a guarded buffer of its own `residue` (+ its index) bytes past a 16-byte
    boundary, `cap` bytes long; the digest array lies between guards at an odd address.  Returns the list of digests; asserts that
    the inputs and all guards are intact, i.e. that exactly 32 n bytes changed."""
    n = len(jobs)
    arr = (Job * max(n, 1))()
    bufs = []
    for i, j in enumerate(jobs):
        room = j["data"][:j["cap"]]
        b = _emu.Guarded(j["cap"], (residue + i) % 16, data=room)
        bufs.append((b, room))
        arr[i].out = None if j["null"] else b.addr
        arr[i].out_cap = j["cap"]
        arr[i].out_len = j["out_len"]
        arr[i].status = j["status"]
    dg = _emu.Guarded(32 * n, digest_residue, fill=0x5A, data=b"\x5A" * (32 * n))
    assert dg.addr % 2 == 1
    lib.emu_sha256_jobs(arr, n, C.c_void_p(dg.addr))
    dg.check("the digest array")
    for i, (b, room) in enumerate(bufs):
        b.check("job %d" % i)
        assert b.read() == room, "job %d: the hashed bytes changed" % i
        assert arr[i].status == jobs[i]["status"] and arr[i].out_len == jobs[i]["out_len"], "job %d: the record changed" % i
    raw = dg.read()
    return [raw[32 * i:32 * i + 32] for i in range(n)]
