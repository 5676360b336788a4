"""CPU tier of the LZ4 block reader's checks: the host build of the lane decoder (csrc/lz4_lane.h) and of the wave parser
(csrc/lz4_wave.h: the checked step, the sub-chunk rounds) with its copiers and the chain walk, on the blocks of _lz4_reader_cases --
one on either side of every comparison of LZ4.process(block:_:) (reference Sources/LZ4/LZ4.swift:332-413) -- against the statuses
stated there by hand and the oracle's bytes."""
import ctypes as C

import pytest

import _emu
import _emu_lz4_linked as E
import _lz4_reader_cases as R
import _oracle as O

CASES = R.all_cases()
FLAT = [c for c in CASES if c.history in ("dict", "none")]      # one job each, through _emu.lz4_block
CHAINS = [c for c in CASES if c.history in ("prefix", "linked")]  # history in place, through the launch of _emu_lz4_linked
GROUP_B = [c for c in CASES if c.name.startswith("B-")]


def _interleaved(flat):
    """Dictionary jobs and the others in turn, as far as the others last."""
    d, o = [c for c in flat if c.history == "dict"], [c for c in flat if c.history != "dict"]
    step = max(len(d) // max(len(o), 1), 1)
    out = []
    for i, c in enumerate(d):
        out.append(c)
        if i % step == 0 and i // step < len(o):
            out.append(o[i // step])
    assert len(out) == len(flat)
    return out


def test_oracle_agrees_with_the_stated_statuses():
    """Every case's status was written down from the Swift; the oracle -- asked with an output limit none of these blocks comes near
    -- must say the same (and SWC_E_CAPACITY is the case's capacity below the oracle's length).  No case is left out."""
    O.lib.refcpu_set_max_output(1 << 30)
    skipped = 0
    for c in CASES:
        if R.oracle_raw(c)[0] == R.CAPACITY:
            skipped += 1
            continue
        assert R.expected(c)[0] == c.status, c.name
    assert skipped == 0
    # both sides of every comparison are there
    for st in (R.OK, R.TRUNCATED, R.CORRUPTED, R.CAPACITY):
        assert any(c.status == st for c in CASES if c.history == "dict")
    for h in ("none", "prefix", "linked"):
        assert {c.status for c in GROUP_B if c.history == h} == {R.OK, R.CORRUPTED}
    assert {len(c.hist) for c in CASES if c.history == "dict"} == set(R.DICT_LENGTHS)


@pytest.fixture(params=[2, 1], ids=["derived-offsets", "eight-byte-records"])
def record_mode(request):
    _emu.lib.emu_set_lz4_record_mode(request.param)
    yield request.param
    _emu.lib.emu_set_lz4_record_mode(2)


@pytest.fixture(params=[1, 0], ids=["wave-copier", "workgroup-resolver"])
def copier(request):
    _emu.lib.emu_set_copier(request.param)
    yield request.param
    _emu.lib.emu_set_copier(1)


@pytest.fixture(params=[0, 2], ids=["forward", "shuffled"])
def order(request):
    _emu.set_order(request.param)
    yield request.param
    _emu.set_order(0)


def test_dictionary_and_plain_jobs(record_mode, copier, order):
    """Group A (dictionaries somewhere else: the lane decoder) and the blocks without history, interleaved in one launch: outputs at
    residues 0 and 5, inputs and dictionaries between guards at residue 3 (10 for the dictionaries), checked unchanged; of an output
    buffer nothing behind min(out_len, capacity) may be written (`exact`: what unwritten_intact() asks on the GPU tier)."""
    cases = _interleaved(FLAT)
    for misalign in (0, 5):
        res = _emu.lz4_block([c.block for c in cases], [c.cap for c in cases], dicts=[c.hist if c.history == "dict" else None for c in cases],
                             misalign=misalign, in_misalign=3, exact=True)
        for c, (st, data, cons, n) in zip(cases, res):
            R.verdict(c, st, n, cons, data)


def test_history_in_place(record_mode, copier, order):
    """Group B behind an adjacent prefix and behind a linked predecessor: one launch over all chains."""
    chains = [R.chain_of(c) for c in CHAINS]
    for misalign in (0, 5):
        for c, res in zip(CHAINS, E.run_chains(chains, misalign=misalign, copier=copier, exact=True)):
            st, n, cons, rel, data = res[-1]
            if c.history == "linked":
                assert res[0][0] == R.OK and res[0][4] == c.hist and rel == len(c.hist), c.name
            R.verdict(c, st, n, cons, data)


def _stats(reset=True):
    st = (C.c_uint64 * 8)()
    _emu.lib.emu_lz4_stats(st, C.c_int(1 if reset else 0))
    return list(st)


def test_rounds_took_the_sequences(record_mode):
    """The blocks of group B are there for the sub-chunk rounds: every one of about 1 KiB started rounds (g_lz4_stats[0]), and the
    rounds took sequences of it (g_lz4_stats[3]).  Only a round that finds an offset beyond the history refuses all it parsed and
    leaves the block to the checked step; in a linked job no round can tell, the chain walk judges the reach."""
    big = [c for c in GROUP_B if len(c.block) >= 900]
    assert len(big) == 3 * 8
    for c in big:
        _stats()
        res = E.run_chain(R.chain_of(c))
        s = _stats()
        R.verdict(c, res[-1][0], res[-1][1], res[-1][2], res[-1][4])
        assert s[0] > 0, c.name + ": no round ran"
        if "reach-beyond" not in c.name or c.history == "linked":
            assert s[3] > 0, c.name + ": the rounds took nothing"
