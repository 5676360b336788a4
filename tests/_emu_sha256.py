"""SHA-256 by one lane per job (csrc/sha256_lane.h, the body of csrc/job_kernels.h) on the host emulation: the binding of
tests/host_emu/emu_sha256.cpp, a library of its own built with _emu's recipe.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import _emu
from _emu import Job
from _sha256_cases import LENGTHS, message, mix  # noqa: F401

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emu")
_LIB = os.path.join(_DIR, "libswc_emu_sha256.so")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "swcompression_amd", "csrc")

def build():
    srcs = [os.path.join(_DIR, f) for f in os.listdir(_DIR) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")]
    if os.path.exists(_LIB) and all(os.path.getmtime(_LIB) >= os.path.getmtime(s) for s in srcs):
        return
    tmp = "%s.%d.tmp" % (_LIB, os.getpid())
    _emu._compile(tmp, "emu_sha256.cpp", ("-O2", "-g"), ("-fPIC", "-shared"))
    os.replace(tmp, _LIB)


build()
lib = C.CDLL(_LIB)
lib.emu_sha256_jobs.argtypes = [C.POINTER(Job), C.c_size_t, C.c_void_p]
lib.emu_sha256_jobs.restype = None


def compile_program(out):
    """The stand-alone program of emu_sha256.cpp (its own main), with the address and undefined-behaviour sanitizers."""
    _emu.compile_program(out, "emu_sha256.cpp", "EMU_SHA256_MAIN")


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
