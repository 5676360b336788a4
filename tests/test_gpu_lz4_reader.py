"""GPU tier of the LZ4 block reader's checks: the blocks of _lz4_reader_cases -- one on either side of every comparison of
LZ4.process(block:_:) (reference Sources/LZ4/LZ4.swift:332-413) -- in ONE launch of swc_batch_decompress_ws on the MI355X, the jobs of
the lane kernel (a dictionary somewhere else) in turn with those of the wave parser (no history, an adjacent prefix, a linked
predecessor), and the dictionary blocks once more as frames through swc_lz4_decompress: against the statuses stated by hand and the
oracle's bytes."""
import pytest

import _lz4_linked_cases as K
import _lz4_reader_cases as R
import _oracle as O
import swcompression_amd as swc
from swcompression_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu

LANE_JOBS_MIN = 130   # one job per lane: two full waves of the lane kernel and a part of a third


@pytest.fixture(autouse=True, params=["auto", "wave"])
def lz_copy_kernel(request):
    """As in test_gpu_lz4.py: the library's own choice of the phase-2 kernels (a launch of fewer than 2,560 jobs: the workgroup
    resolver for the jobs without history), and the wave copier forced for all."""
    from swcompression_amd import _lib
    lib = _lib.load()
    assert lib.swc_set_tuning(b"lz_copier", -1 if request.param == "wave" else 1) == 0
    yield request.param
    lib.swc_set_tuning(b"lz_copier", 1)


def launch_order():
    """The cases in the order of the launch: a dictionary job, one of the others, a dictionary job, ... -- the list of dictionary
    cases repeated until it has LANE_JOBS_MIN jobs, the others as often as that takes."""
    d = [c for c in R.all_cases() if c.history == "dict"]
    o = [c for c in R.all_cases() if c.history != "dict"]
    d = d * -(-LANE_JOBS_MIN // len(d))
    assert len(d) >= LANE_JOBS_MIN and len(d) >= len(o)
    out = []
    for i, c in enumerate(d):
        out += [c, o[i % len(o)]]
    return out


def test_one_launch():
    cases = launch_order()
    chains = [K.chain(c.name, [K.J(c.block, c.cap, 0, c.hist)]) if c.history == "dict" else R.chain_of(c) for c in cases]
    jobs = [j for ch in chains for j in ch["jobs"]]
    prefixes = [ch["prefix"] if k == 0 and ch["prefix"] else None for ch in chains for k in range(len(ch["jobs"]))]
    b = DeviceBatch("lz4_block", [j["data"] for j in jobs], [j["cap"] for j in jobs], aux=[j["aux"] for j in jobs],
                    dicts=[j["dict"] for j in jobs], prefixes=prefixes, guard=16)
    b.launch(sync=True)
    r = b.results()
    blob = b.d_out.cpu().numpy()
    base = b.d_out.data_ptr()

    def job(i):
        at = int(r["out"][i]) - base
        kept = int(min(r["out_len"][i], r["out_cap"][i]))
        assert 0 <= at and at + kept <= blob.size - 16, "job %d: `out` points outside the batch's output buffer" % i
        return int(r["status"][i]), int(r["out_len"][i]), int(r["in_consumed"][i]), blob[at:at + kept].tobytes()

    i = 0
    for c, ch in zip(cases, chains):
        assert int(r["out"][i]) - base == int(b._out_off[i]), c.name + ": the head's `out` moved"
        if c.history == "linked":
            st, n, cons, data = job(i)
            assert (st, n, data) == (R.OK, len(c.hist), c.hist), c.name + ": the predecessor"
            i += 1
            assert int(r["out"][i]) - base == int(b._out_off[i - 1]) + len(c.hist), c.name + ": `out` is not behind the predecessor's output"
        st, n, cons, data = job(i)
        R.verdict(c, st, n, cons, data)
        i += 1
    assert i == b.n
    assert b.unwritten_intact(), "bytes outside the jobs' outputs were written"


def test_dictionary_blocks_as_frames():
    """Group A through swc_lz4_decompress: every block the only one of a frame of independent blocks, with its dictionary -- the
    status or the bytes of the oracle's frame decoder."""
    from swcompression_amd import _lib
    lib = _lib.load()
    seen = set()
    before = lib.swc_stat(b"launches")
    for c in R.all_cases():
        if c.history != "dict" or not c.block or (c.block, len(c.hist)) in seen:   # (a block of no bytes is the frame's end mark)
            continue
        seen.add((c.block, len(c.hist)))
        frame = R.frame_of(c.block)
        st, out, _ = O.lz4(frame, c.hist)
        assert st == (R.OK if c.status == R.CAPACITY else c.status), c.name + ": the frame does not end as its block does"
        if st == 0:
            assert swc.LZ4.decompress(frame, c.hist) == out, c.name
        else:
            with pytest.raises(swc.SWCError) as ei:
                swc.LZ4.decompress(frame, c.hist)
            assert ei.value.status == st, c.name
    assert len(seen) >= LANE_JOBS_MIN
    assert lib.swc_stat(b"launches") - before == len(seen), "a frame's block did not go to the device in a launch of its own"
