"""CPU tier of SHA-256 on the device (csrc/sha256_lane.h: one job per lane; the body of csrc/job_kernels.h that swc_sha256_kernel
runs) in the host emulation, against hashlib, the oracle and the seven known answers the reference's own tests hold; the stand-alone
program under ASan + UBSan with every message at the very end of its allocation: the kernel reads no byte outside out[0 .. len)."""
import hashlib
import json
import os
import struct

import pytest

import _emu
import _emu_sha256 as E
import _oracle as O

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_inline_vectors.json")))


def _job(data, **kw):
    j = {"data": data, "cap": len(data), "out_len": len(data), "status": 0, "null": False}
    j.update(kw)
    return j


@pytest.mark.parametrize("vec", GOLD["sha256"], ids=lambda v: v["hash"][:8])
def test_reference_known_answers(vec):
    x = vec["input"].encode()
    assert E.run([_job(x)])[0].hex() == vec["hash"]


@pytest.mark.parametrize("n", E.LENGTHS)
def test_every_length_at_every_residue(n):
    """One message per tail path, at all 16 residues of its address, in guarded buffers; hashlib and the oracle agree."""
    x = E.message(n)
    want = hashlib.sha256(x).digest()
    assert O.sha256(x) == want
    for res in range(16):
        assert E.run([_job(x)], residue=res, digest_residue=2 * res + 1)[0] == want, "length %d at residue %d" % (n, res)
    if n == 0:
        assert E.run([_job(b"", null=True)])[0] == want   # nothing to read: `out` may be null


@pytest.mark.parametrize("n", [130, 1, 63, 64, 65])
def test_launch_of_mixed_jobs(n):
    """One launch whose lanes differ in their block counts: zero-length jobs with a null `out`, a job that needed more than its
    capacity (the digest covers out_cap bytes), a job with an error status (hashed like any other)."""
    jobs = E.mix()[:n]
    got = E.run(jobs, residue=3, digest_residue=7)
    for i, (j, g) in enumerate(zip(jobs, got)):
        assert g == hashlib.sha256(j["want"]).digest(), "job %d of %d (%d bytes)" % (i, n, len(j["want"]))
    if n == 130:
        assert len(jobs[9]["want"]) == jobs[9]["cap"] < jobs[9]["out_len"] and jobs[70]["status"] != 0
        assert sum(1 for j in jobs if j["null"]) == 3 and len({(len(j["want"]) + 8) // 64 for j in jobs[:64]}) > 8


def test_standalone_program_sanitized(tmp_path):
    """tests/host_emu/emu_sha256.cpp as a program of its own under ASan + UBSan: every length at the 16 residues, the message the last
    bytes of its heap allocation, alone and as one lane of a launch of all lengths; a byte read behind a message is a heap overflow."""
    cases = struct.pack("<I", len(E.LENGTHS)) + b"".join(struct.pack("<I", n) + hashlib.sha256(E.message(n)).digest() for n in E.LENGTHS)
    out = _emu.run_program(tmp_path, "emu_sha256.cpp", "EMU_SHA256_MAIN", cases)
    assert "%d lengths at 16 residues, 0 mismatches" % len(E.LENGTHS) in out
