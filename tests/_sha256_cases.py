"""The messages and job lists both tiers hash (tests/test_sha256_emulation.py, tests/test_gpu_sha256.py).  TEST INFRASTRUCTURE ONLY."""
import random

# every length at which the tail takes another path: none, bytes only, dwords and bytes, the marker in the last free byte (55), the
# second padding block (56 .. 63), whole blocks with and without a tail, several blocks
LENGTHS = (0, 1, 3, 4, 5, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 191, 192, 1000, 4113, 65591)


def message(n):
    """The message of n bytes that emu_sha256_message of tests/host_emu/emu_sha256.cpp writes."""
    x = 0x9E3779B9 ^ (n & 0xFFFFFFFF)
    out = bytearray(n)
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = x >> 24
    return bytes(out)


def mix(seed=0):
    """The 130 jobs of one launch, as dicts data / cap / out_len / status / null: the lengths of LENGTHS mixed so that the lanes of a
    wave differ in their block counts, jobs of no bytes with a null `out`, one job that needed more than its capacity (what exists
    is out_cap bytes), one with an error status.  `want` is the message the digest covers."""
    rng = random.Random(1234 + seed)
    jobs = []
    for i in range(130):
        n = LENGTHS[(i * 7 + seed) % len(LENGTHS)] if i % 4 else rng.randrange(0, 700)
        data = rng.randbytes(n)
        jobs.append({"data": data, "cap": n, "out_len": n, "status": 0, "null": False, "want": data})
    for i in (5, 64, 129):
        jobs[i].update(data=b"", cap=0, out_len=0, null=True, want=b"")
    jobs[9].update(cap=len(jobs[9]["data"]) // 2 + 1, out_len=len(jobs[9]["data"]) + 77)
    jobs[9]["want"] = jobs[9]["data"][:jobs[9]["cap"]]
    jobs[70]["status"] = 104
    return jobs
