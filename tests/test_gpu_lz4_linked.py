"""GPU tier of the linked LZ4 blocks: chains of SWC_LZ4_LINKED / SWC_LZ4_STORED jobs and adjacent prefixes through
swc_batch_decompress_ws, and linked frames through the single-shot entry points, on the MI355X vs the oracle -- block by block
with the 64 KiB suffix rule (_lz4_linked_cases.expect) and frame by frame (_oracle.lz4)."""
import numpy as np
import pytest

import _lz4_build as LB
import _lz4_linked_cases as K
import _oracle as O
import swcompression_amd as swc
from swcompression_amd import _lib, corpus
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu


def build_batch(chains):
    """One batch over the jobs of `chains`, in order; 16 guard bytes of 0xA5 around every chain's buffer."""
    jobs = [j for ch in chains for j in ch["jobs"]]
    prefixes = [ch["prefix"] if k == 0 and ch["prefix"] else None for ch in chains for k in range(len(ch["jobs"]))]
    return DeviceBatch("lz4_block", [j["data"] for j in jobs], [j["cap"] for j in jobs], aux=[j["aux"] for j in jobs],
                       dicts=[j["dict"] for j in jobs], prefixes=prefixes, guard=16)


def check_batch(b, chains, expected=K.expected):
    """Every job of every chain vs the oracle: status, out_len, in_consumed, the written-back `out`, the bytes; the guards."""
    r = b.results()
    blob = b.d_out.cpu().numpy()
    base = b.d_out.data_ptr()
    i = 0
    for ch in chains:
        exp = expected(ch)
        at = int(r["out"][i]) - base
        assert at == int(b._out_off[i]), ch["name"] + ": the head's `out` moved"
        for k, (st, out, n) in enumerate(exp):
            what = "%s job %d" % (ch["name"], k)
            assert int(r["status"][i]) == st, what
            if ch.get("orphans") and k:   # (refused jobs: `out` is nobody's to set)
                assert int(r["out_len"][i]) == 0 and int(r["in_consumed"][i]) == 0, what
                i += 1
                continue
            assert int(r["out"][i]) - base == at, what + ": `out` is not behind the predecessor's output"
            if n is not None:
                assert int(r["out_len"][i]) == n, what
            if st == K.OK:
                assert int(r["in_consumed"][i]) == len(ch["jobs"][k]["data"]), what
                assert blob[at:at + n].tobytes() == out, what
            at += int(min(r["out_len"][i], r["out_cap"][i]))
            i += 1
    assert i == b.n
    assert b.unwritten_intact(), "bytes outside the jobs' outputs were written"


def test_batch_api_cases():
    """Cases 1-8 of the CPU tier in ONE batch.  Without the feature `aux` is ignored: the second block of the first case has no
    history and ends with SWC_E_DATA_CORRUPTED."""
    chains = K.all_cases()
    b = build_batch(chains)
    b.launch(sync=True)
    check_batch(b, chains)


def test_orphans_are_refused():
    """A launch whose job 0 is linked, and a head of the lane decoder with linked jobs behind it: SWC_E_INVALID_ARGUMENT with nothing
    produced for every linked job no head can carry, the oracle's bytes for everybody else in the launch."""
    by = {c["name"]: c for c in K.all_cases()}
    chains = [K.orphan_job0(), by["seam-inside"], K.orphan_behind_lane_head(), by["tiny-5-7-100"]]
    b = build_batch(chains)
    b.launch(sync=True)
    r = b.results()
    assert [int(x) for x in r["status"][:2]] == [K.INVALID_ARGUMENT] * 2 and [int(x) for x in r["out_len"][:2]] == [0, 0]
    check_batch(b, chains)


def mixed_chains():
    by = {c["name"]: c for c in K.all_cases()}
    plain = [K.chain("independent-%d" % i, [K.J(corpus.lz4_block(corpus.p_text(3000 + 97 * i, 200 + i)), 3000 + 97 * i)]) for i in range(10)]
    d = corpus.p_text(5000, 210)
    with_dict = K.chain("dictionary-elsewhere", [K.J(LB.block([(b"abc", 4000, 40)] + K._filler(20, 211), corpus.p_text(12, 212)), 1024, 0, d)])
    stored = K.chain("stored-alone", [K.J(corpus.p_rand(777, 213), 777, K.STORED)])
    return plain[:5] + [by["seam-over"], with_dict] + plain[5:] + [by["liblz4-quarter-random-4"], stored]


def expected_mixed(ch):
    if ch["name"] == "dictionary-elsewhere":   # (a prefix that is not in place: expect() knows adjacent ones only)
        j = ch["jobs"][0]
        st, out = O.lz4_block(j["data"], j["dict"])
        return [(st, out, len(out))]
    return K.expected(ch)


@pytest.mark.parametrize("copier", [1, -1])
def test_mixed_launch(copier):
    """Independent blocks, two chains, a dictionary that is not adjacent and a stored job in one launch of fewer than 2,560 jobs:
    three kernels share the jobs (lane decoder; parse + workgroup resolver; record-mode parse + wave copier), and with lz_copier
    = -1 two do."""
    lib = _lib.load()
    chains = mixed_chains()
    assert lib.swc_set_tuning(b"lz_copier", copier) == 0
    try:
        b = build_batch(chains)
        assert b.n < 2560
        b.launch(sync=True)
        check_batch(b, chains, expected_mixed)
    finally:
        lib.swc_set_tuning(b"lz_copier", 1)


def test_many_chains():
    """2,600 chains of three blocks of 1 KiB -- above the threshold of the wave copier and of the launch order: one wave per chain."""
    distinct = []
    for c in range(16):
        first = K.lits_block(1024, 300 + c)
        lit = corpus.p_text(8 * 31 + 32, 320 + c)
        second = LB.block([(lit[8 * i:8 * i + 8], 33 * i + 40 + c, 24) for i in range(31)], lit[-32:])                  # into the first block
        third = LB.block([(lit[8 * i:8 * i + 8], 1024 + 32 * i + 9 + c, 24) for i in range(31)], lit[-32:])            # ... over the second
        distinct.append(K.chain("many-%d" % c, [K.J(first, 1024), K.J(second, 1024, K.LINKED), K.J(third, 1024, K.LINKED)]))
    exp = [K.expect(ch) for ch in distinct]
    assert all(st == K.OK and len(out) == 1024 for e in exp for st, out, _ in e)
    want = [b"".join(out for _, out, _ in e) for e in exp]
    reps = 2600
    jobs = [j for r in range(reps) for j in distinct[r % 16]["jobs"]]
    b = DeviceBatch("lz4_block", [j["data"] for j in jobs], [1024] * len(jobs), aux=[j["aux"] for j in jobs])
    assert b.n == 7800
    b.launch(sync=True)
    r = b.results()
    assert (r["status"] == 0).all() and (r["out_len"] == 1024).all()
    assert (r["out"] - np.uint64(b.d_out.data_ptr()) == b._out_off.astype(np.uint64)).all()      # 1 KiB each: nothing moved
    blob = b.d_out.cpu().numpy()[:3072 * reps].reshape(reps, 3072)
    for c in range(16):
        assert (blob[c::16] == np.frombuffer(want[c], dtype=np.uint8)).all(), "chain %d" % c


def _decompress(lib, frame, dictionary=None):
    """swc_lz4_decompress as the C ABI returns it: (status, bytes)."""
    import ctypes as C
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t()
    used = C.c_size_t()
    d = None if dictionary is None else bytes(dictionary)
    st = lib.swc_lz4_decompress(bytes(frame), len(frame), d, 0 if d is None else len(d), -1, C.byref(out), C.byref(n), C.byref(used))
    data = C.string_at(out, n.value) if n.value else b""
    lib.swc_free(out)
    return st, data


def linked_frame(name):
    """(payload, frame of five linked blocks of 64 KiB, dictionary)."""
    payload = corpus.p_text(5 * 65536 - 1000, 400)
    if name == "plain":
        return payload, corpus.lz4f_frame(payload, 4, True, True), None
    if name == "block-checksums":
        return payload, corpus.lz4f_frame(payload, 4, True, True, True, True), None
    # a linked frame whose first block references a dictionary: the engine's own compressor writes one; the oracle reads it
    d = corpus.p_text(70000, 401)
    return payload, swc.LZ4.compress(payload, independent_blocks=False, block_size=65536, dictionary=d), d


@pytest.mark.parametrize("name", ["plain", "block-checksums", "dictionary"])
def test_single_frame(name):
    """A linked frame of five blocks through swc_lz4_decompress: the oracle's bytes in exactly ONE launch (block by block it took
    five), and the oracle's status and output on the frame truncated at every 4,099th byte."""
    payload, frame, d = linked_frame(name)
    lib = _lib.load()
    assert swc.index_blocks("lz4", frame, flags=True)[4][4] == 1 and len(swc.index_blocks("lz4", frame)) == 5
    st, out, _ = O.lz4(frame, d)
    assert st == 0 and out == payload
    before = lib.swc_stat(b"launches")
    assert _decompress(lib, frame, d) == (0, out)
    assert lib.swc_stat(b"launches") - before == 1
    for cut in range(4099, len(frame), 4099):
        est, eout, _ = O.lz4(frame[:cut], d)
        assert _decompress(lib, frame[:cut], d) == (est, eout if est in (0, 503) else b""), "truncated at %d" % cut   # (only checksumMismatch carries output)


def test_many_and_multi():
    """swc_unarchive_many over 64 linked frames interleaved with 64 independent ones: one launch, every archive the oracle's; and
    swc_lz4_multi_decompress over three linked frames."""
    lib = _lib.load()
    frames = []
    for i in range(64):
        p = corpus.p_text(70000 + 1111 * (i % 7), 500 + i)          # two blocks of 64 KiB
        frames.append(corpus.lz4f_frame(p, 4, True, i % 2 == 0))
        frames.append(corpus.lz4f_frame(p[::-1], 4, False, True))
    frames[10] = frames[10][:-9]                                      # a linked frame cut short: its own error, nobody else's
    exp = [O.lz4(f) for f in frames]
    before = lib.swc_stat(b"launches")
    got = swc.unarchive_many("lz4", frames)
    assert lib.swc_stat(b"launches") - before == 1
    for i, ((st, out, _), (gst, gout)) in enumerate(zip(exp, got)):
        assert (gst, gout) == (st, out if st in (0, 503) else b""), i
    three = [corpus.lz4f_frame(corpus.p_text(140000, 600 + i), 4, True, True) for i in range(3)]
    est, eouts = O.lz4_multi(b"".join(three))
    assert est == 0
    before = lib.swc_stat(b"launches")
    assert swc.LZ4.multi_decompress(b"".join(three)) == eouts
    assert lib.swc_stat(b"launches") - before == 1
