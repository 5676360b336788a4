"""CPU tier of the linked LZ4 blocks: the host build of the parse with history (csrc/lz4_wave.h), the copier with history
(csrc/lz_copy.h) and the chain walk (csrc/lz4_chain.h) -- tests/host_emu/emu_lz4_linked.cpp -- against the oracle, block by block
with the 64 KiB suffix rule: in three lane orders, with the head's output at every misalignment, guard bytes on both sides."""
import pytest

import _emu
import _emu_lz4_linked as E
import _lz4_linked_cases as K
import _oracle as O
from swcompression_amd import corpus

CASES = K.all_cases()
ORDERS = (0, 1, 2)


def check(ch, res):
    exp = K.expected(ch)
    at = 0
    for k, ((st, out, n), (gst, glen, gcons, grel, gbytes)) in enumerate(zip(exp, res)):
        what = "%s job %d" % (ch["name"], k)
        assert gst == st, what
        if ch.get("orphans") and k:   # (refused jobs: `out` is nobody's to set)
            assert glen == 0 and gcons == 0, what
            continue
        assert grel == at, what + ": `out` is not behind the predecessor's output"
        if n is not None:
            assert glen == n, what
        if st == K.OK:
            assert gbytes == out, what
            assert gcons == len(ch["jobs"][k]["data"]), what
            at += n
        else:   # (the next job's `out` lies behind the bytes of this one that exist)
            at += min(glen, ch["jobs"][k]["cap"])


def small(ch):
    return sum(j["cap"] for j in ch["jobs"]) <= 8192


@pytest.mark.parametrize("ch", CASES, ids=[c["name"] for c in CASES])
def test_chain_against_oracle(ch):
    """Every case at every misalignment 0..15 of the head's output in lane order forward, and in the other two orders the small ones
    at all sixteen, the large ones at four."""
    for order in ORDERS:
        E.set_order(order)
        for mis in (range(16) if small(ch) or order == 0 else (0, 1, 9, 15)):
            check(ch, E.run_chain(ch, misalign=mis))
    E.set_order(0)


def test_reach_statuses():
    """What the cases of the reach check must come to, spelled out (the oracle agrees: test_chain_against_oracle)."""
    by = {c["name"]: c for c in CASES}
    for tag in ("-step", "-rounds"):
        assert [r[0] for r in E.run_chain(by["reach-exact" + tag])] == [K.OK] * 3
        for name in ("reach-beyond", "reach-beyond-truncated"):
            res = E.run_chain(by[name + tag])
            assert [r[0] for r in res] == [K.OK, K.CORRUPTED, K.CORRUPTED]
            assert [r[1] for r in res[1:]] == [0, 0]
            assert res[0][4] == K.expected(by[name + tag])[0][1]
        # the truncation alone is the other error: the reach is what comes first
        cut = by["reach-beyond-truncated" + tag]["jobs"][1]["data"]
        assert O.lz4_block(cut, b"\0" * 400)[0] == K.TRUNCATED
    assert [r[0] for r in E.run_chain(by["reach-64k"])] == [K.OK] * 3


def test_argument_and_capacity_errors():
    by = {c["name"]: c for c in CASES}
    res = E.run_chain(by["linked-with-dict"])
    assert [r[0] for r in res] == [K.OK, K.INVALID_ARGUMENT, K.INVALID_ARGUMENT] and [r[1] for r in res[1:]] == [0, 0]
    res = E.run_chain(by["stored-capacity"])
    assert [r[0] for r in res] == [K.OK, K.CAPACITY, K.CAPACITY] and [r[1] for r in res[1:]] == [40, 0]


def test_orphans_are_refused():
    """Linked jobs that no head can carry report SWC_E_INVALID_ARGUMENT with nothing produced -- never the parse's SWC_OK for bytes
    nobody wrote: behind a head whose prefix is not in place (the head itself decodes), and from job 0 on."""
    for order in ORDERS:
        E.set_order(order)
        res = E.run_chain(K.orphan_behind_lane_head())
        assert [r[:3] for r in res[1:]] == [(K.INVALID_ARGUMENT, 0, 0)] * 2 and res[0][0] == K.OK
        assert res[0][4] == K.expected(K.orphan_behind_lane_head())[0][1]
        ch = K.orphan_job0()
        res = E.run_chain(ch)
        assert [r[:3] for r in res] == [(K.INVALID_ARGUMENT, 0, 0)] * 2
        check(ch, res)
    E.set_order(0)


def split_launch():
    """One job list with a job for every kernel of a launch below kCopierMin: a plain block, a block with a dictionary somewhere
    else, one with an adjacent prefix, a chain of three linked blocks, a stored block, a block that fails."""
    by = {c["name"]: c for c in CASES}
    plain = corpus.lz4_block(corpus.p_text(3000, 5))
    lane = K.orphan_behind_lane_head()
    lane = dict(lane, name="split-dictionary-elsewhere", jobs=lane["jobs"][:1])
    return [K.chain("split-plain", [K.J(plain, 3000)]), lane, dict(by["prefix-first-byte"]), dict(by["reach-exact-step"]),
            K.chain("split-stored", [K.J(b"stored as it is", 15, K.STORED)]), K.chain("split-fails", [K.J(plain[:len(plain) - 7], 3000)])]


def test_small_launch_split():
    """A launch below kCopierMin splits its jobs over four kernels (parse without records, record-mode parse, byte-cell resolver,
    chain copier), a larger one runs one parse and the chain copier: both against the oracle in the three lane orders, both leave the
    same job records, the guards around every output are intact (run_chains), and the decoding paths took every job exactly once
    between them -- all results are right, so none was skipped, and the paths' count is the number of jobs."""
    chains = split_launch()
    n = sum(len(ch["jobs"]) for ch in chains)
    assert K.expected(chains[-1])[0][0] != K.OK and all(e[0] == K.OK for ch in chains[:-1] for e in K.expected(ch))
    for order in ORDERS:
        E.set_order(order)
        try:
            got = {}
            for copier in (0, 1):
                E.jobs_taken()
                got[copier] = E.run_chains(chains, misalign=3, copier=copier)
                assert E.jobs_taken() == n, "copier %d, order %d" % (copier, order)
                for ch, res in zip(chains, got[copier]):
                    check(ch, res)
        finally:
            E.set_order(0)
        for ch, small, large in zip(chains, got[0], got[1]):
            assert [r[:4] for r in small] == [r[:4] for r in large], ch["name"]
            if K.expected(ch)[0][0] == K.OK:
                assert [r[4] for r in small] == [r[4] for r in large], ch["name"]


def test_frames_whole():
    """The liblz4 frames once more against the oracle's frame decoder: the chain's bytes are the frame's."""
    for ch in K.liblz4_cases():
        tag = ch["name"].split("-", 1)[1].rsplit("-", 1)
        payload = K.liblz4_payloads()[tag[0]]
        res = E.run_chain(ch)
        assert all(r[0] == K.OK for r in res)
        assert b"".join(r[4] for r in res) == payload
        if ch["name"] == "liblz4-quarter-random-4":
            assert any(j["aux"] & K.STORED for j in ch["jobs"]), "the case was meant to hold stored blocks"


def test_stand_alone_program_with_sanitizers(tmp_path):
    """Cases 1-6 in a program of its own, built with the address and undefined-behaviour sanitizers: every chain in exactly the
    bytes the job contract names, at sixteen alignments, in three lane orders."""
    def exp(ch):
        return [(st, out, 0 if n is None else n) for st, out, n in K.expected(ch)]
    _emu.run_program(tmp_path, "emu_lz4_linked.cpp", "EMU_LZ4_LINKED_MAIN", E.case_file(K.sanitizer_cases(), exp))


def test_index_blocks_flags():
    """swc_index_blocks kind 4 (host only): flags bit 0 on every block of a linked frame but the first, 0 for independent blocks;
    aux = 1 on the stored ones.  What the index says is what the frame holds (the parser of the cases)."""
    import swcompression_amd as swc
    payload = K.liblz4_payloads()["quarter-random"]
    for linked in (True, False):
        frame = corpus.lz4f_frame(payload, block_size_code=4, linked=linked)
        refs = swc.index_blocks("lz4", frame, flags=True)
        _, blocks = K.frame_blocks(frame)
        assert len(refs) == len(blocks) == 4
        assert [r[4] for r in refs] == ([0, 1, 1, 1] if linked else [0, 0, 0, 0])
        assert [(frame[r[0]:r[0] + r[1]], bool(r[3])) for r in refs] == blocks
        assert swc.index_blocks("lz4", frame) == [r[:4] for r in refs]
