"""GPU tier of SHA-256 on the device: swc_batch_sha256 (one job per lane, csrc/sha256_lane.h) against hashlib at every tail length and
all 16 residues; the XZ walk taking the digests of a --check=sha256 file from the launch that decoded its blocks ahead
("sha256_device_min_units"); swc_unarchive_many("xz") decoding the blocks of a whole set of archives in one launch."""
import ctypes as C
import hashlib
import lzma

import numpy as np
import pytest

import _oracle as O
import _placed as P
import _sha256_cases as K
import _xz_build as X
import swcompression_amd as swc
from swcompression_amd import _lib, corpus
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu

WRONG_CHECK = 807
MIN_UNITS_DEFAULT = 32   # what the library ships for "sha256_device_min_units" (include/swc_hip.h)
KEY = b"sha256_device_min_units"


def _stat(key):
    return _lib.load().swc_stat(key)


def _device_digests(jobs, residue):
    """The jobs (dicts of _sha256_cases.mix) laid out by the placement harness -- job i's bytes at residue (residue + i) % 16, between
    guards -- and hashed by swc_batch_sha256 into a guarded array at an odd address.  Asserts that nothing but the 32 n bytes changed."""
    import torch
    n = len(jobs)
    res = [(residue + i) % 16 for i in range(n)]
    pb = P.PlacedBatch("delta", [j["data"][:j["cap"]] for j in jobs], [j["cap"] for j in jobs], [0] * n, res, in_place=[True] * n)
    rec = pb.jobs_host.copy()
    rec["out_len"] = [j["out_len"] for j in jobs]
    rec["status"] = [j["status"] for j in jobs]
    for i, j in enumerate(jobs):
        if j["null"]:
            rec["in"][i] = rec["out"][i] = 0
    d_jobs = torch.from_numpy(rec.view(np.uint8).copy()).to(pb.device)
    guard = 64
    d_dg = torch.full((guard + 1 + 32 * n + guard,), 0x5A, dtype=torch.uint8, device=pb.device)
    at = guard + 1 if d_dg.data_ptr() % 2 == 0 else guard
    assert (d_dg.data_ptr() + at) % 2 == 1
    opts = pb._opts()
    st = pb.lib.swc_batch_sha256(d_jobs.data_ptr(), n, d_dg.data_ptr() + at, C.byref(opts))
    assert st == 0, "swc_batch_sha256 failed with status %d" % st
    torch.cuda.synchronize(pb.device)
    got = d_dg.cpu().numpy()
    assert (got[:at] == 0x5A).all() and (got[at + 32 * n:] == 0x5A).all(), "bytes outside the digest array changed"
    assert (pb.d_out.cpu().numpy() == pb.out_host).all(), "the hashed buffer changed"
    assert d_jobs.cpu().numpy().tobytes() == rec.tobytes(), "the job records changed"
    return [got[at + 32 * i:at + 32 * i + 32].tobytes() for i in range(n)]


def test_every_length_at_every_residue():
    msgs = [K.message(n) for n in K.LENGTHS]
    # one launch, sixteen jobs per length: job 16 k + r hashes length k at residue r
    jobs = [{"data": m, "cap": len(m), "out_len": len(m), "status": 0, "null": False} for m in msgs for _ in range(16)]
    got = _device_digests(jobs, residue=0)
    for i, g in enumerate(got):
        assert g == hashlib.sha256(msgs[i // 16]).digest(), "length %d at residue %d" % (len(msgs[i // 16]), i % 16)


@pytest.mark.parametrize("n", [130, 1, 63, 64, 65])
def test_launch_of_mixed_jobs(n):
    jobs = K.mix()[:n]
    got = _device_digests(jobs, residue=5)
    for i, (j, g) in enumerate(zip(jobs, got)):
        assert g == hashlib.sha256(j["want"]).digest(), "job %d of %d (%d bytes)" % (i, n, len(j["want"]))


def test_device_batch_sha256_after_a_decode():
    """DeviceBatch.sha256(): the digests of what a Deflate launch left, an empty and a failed stream among them."""
    plains = [K.message(n) for n in K.LENGTHS] + [corpus.p_text(70000, 3)]
    units = [corpus.deflate_raw(p) for p in plains] + [b"\x07garbage"]
    b = DeviceBatch("deflate", units, [max(len(p), 1) for p in plains] + [64])
    b.launch(sync=True)
    r = b.results()
    d = b.sha256()
    assert d.shape == (len(units), 32) and d.dtype == np.uint8
    assert int(r["status"][-1]) != 0
    for i in range(len(units)):
        made = b.output(i)
        if i < len(plains):
            assert int(r["status"][i]) == 0 and made == plains[i]
        assert d[i].tobytes() == hashlib.sha256(made).digest(), "job %d" % i


def _payload20():
    return corpus.p_text(4096 * 12, 41) + corpus.p_mix(4096 * 7 + 1234, 42)


def test_xz_walk_takes_the_digests_from_the_device():
    lib = _lib.load()
    x = _payload20()
    built = X.build(X.cut(x, 4096), X.CHECK_SHA256)
    assert len(built.blocks) == 20 and O.xz_unarchive(built.stream) == (0, x)
    bad = built.with_damaged_check(7, byte=13, bit=2)
    est, edata = O.xz_unarchive(bad)
    assert est == WRONG_CHECK and edata == x[:8 * 4096]
    try:
        assert lib.swc_set_tuning(KEY, 1) == 0
        units, launches = _stat(b"sha256_device_units"), _stat(b"launches")
        assert swc.XZArchive.unarchive(built.stream) == x
        assert _stat(b"sha256_device_units") - units == 20
        assert _stat(b"launches") - launches <= 2
        units = _stat(b"sha256_device_units")
        with pytest.raises(swc.XZError) as ei:
            swc.XZArchive.unarchive(bad)
        assert ei.value.case == "wrongCheck" and ei.value.data == edata
        assert _stat(b"sha256_device_units") - units == 8   # blocks 0 .. 7: the walk ends at the block whose check fails
        # above the number of blocks: the host computes the digests, as before
        assert lib.swc_set_tuning(KEY, 21) == 0
        units = _stat(b"sha256_device_units")
        assert swc.XZArchive.unarchive(built.stream) == x
        with pytest.raises(swc.XZError) as ei:
            swc.XZArchive.unarchive(bad)
        assert ei.value.case == "wrongCheck" and ei.value.data == edata
        assert _stat(b"sha256_device_units") == units
    finally:
        assert lib.swc_set_tuning(KEY, MIN_UNITS_DEFAULT) == 0


def _archive_set():
    """48 archives: 40 single-block SHA-256 archives of 0 to 70,000 bytes from liblzma -- three of them damaged: a flipped bit in the
    check field, the last bytes cut off, a flipped byte in the LZMA2 data --, four built multi-block SHA-256 archives, three with
    CRC-64 or no check, one empty input.  Returns (archives, the number of SHA-256 blocks that decode cleanly)."""
    sizes = [0, 1, 55, 56, 64, 100, 1000, 4113, 70000, 65591] + [(i * 1877) % 70001 for i in range(1, 28)]
    singles = [lzma.compress(corpus.p_mix(n, 700 + i) if i % 3 else corpus.p_text(n, 700 + i), check=lzma.CHECK_SHA256, preset=1)
               for i, n in enumerate(sizes)]
    clean = sum(1 for n in sizes if n > 0)
    base = lzma.compress(corpus.p_text(30000, 761), check=lzma.CHECK_SHA256, preset=1)
    (off, comp, _, _), = swc.index_blocks("xz", base)
    damaged_check = bytearray(base)
    damaged_check[off + (comp + 3) // 4 * 4 + 9] ^= 0x10
    flipped = bytearray(base)
    flipped[off + comp // 2] ^= 0x04
    singles += [bytes(damaged_check), base[:-5], bytes(flipped)]
    clean += 1                                                  # the damaged check: its block decodes, its digest does not match
    clean += 1 if O.xz_unarchive(bytes(flipped))[0] == WRONG_CHECK else 0   # (if the flipped byte still decodes: to other bytes)
    assert len(singles) == 40
    multi = []
    for k, (n, blk) in enumerate([(20000, 4096), (9000, 1000), (70000, 30000), (5000, 4999)]):
        b = X.build(X.cut(corpus.p_mix(n, 780 + k), blk), X.CHECK_SHA256)
        multi.append(b.stream)
        clean += len(b.blocks)
    others = [lzma.compress(corpus.p_text(12345, 790), check=lzma.CHECK_CRC64, preset=1),
              X.build(X.cut(corpus.p_mix(9000, 791), 2048), X.CHECK_NONE).stream,
              lzma.compress(corpus.p_mix(333, 792), check=lzma.CHECK_NONE, preset=1)]
    archives = singles + multi + others + [b""]
    assert len(archives) == 48
    return archives, clean


def test_unarchive_many_xz_one_launch_for_the_set():
    lib = _lib.load()
    archives, clean = _archive_set()
    expected = [O.xz_unarchive(a) for a in archives]
    assert {st for st, _ in expected} >= {0, WRONG_CHECK} and sum(1 for st, _ in expected if st not in (0, WRONG_CHECK)) >= 1
    try:
        assert lib.swc_set_tuning(KEY, 1) == 0
        units, launches = _stat(b"sha256_device_units"), _stat(b"launches")
        got = swc.unarchive_many("xz", archives)
        assert _stat(b"launches") - launches <= 3, "the blocks of the set must share one launch"
        assert _stat(b"sha256_device_units") - units == clean
        for i, ((st, data), (est, edata)) in enumerate(zip(got, expected)):
            assert st == est, "archive %d: status %d, oracle %d" % (i, st, est)
            assert data == (edata if est in (0, WRONG_CHECK) else b""), "archive %d differs" % i
        # the same set with the digests on the host: the same answers
        assert lib.swc_set_tuning(KEY, 1 << 20) == 0
        units = _stat(b"sha256_device_units")
        assert swc.unarchive_many("xz", archives) == got
        assert _stat(b"sha256_device_units") == units
    finally:
        assert lib.swc_set_tuning(KEY, MIN_UNITS_DEFAULT) == 0
