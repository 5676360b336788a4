"""CPU tier: the chain check of a sub-chunk round on its own -- swcompression_amd/csrc/sync_round.h: chain_check, the one
copy that the Deflate rounds (one wave and team helper, fast and general pass) and the LZ4 parse call.  64 lanes' starts, ends,
`have` and flags go in; b (the first lane not decoded from its left neighbour's end), E (the first stopped lane INSIDE the chain)
and nv (E + 1 if there is one, else b) come out and are compared with the definition restated below."""
import random

import pytest

import _emu as E

N = 64
EOB, FAIL = 1, 2   # (two flag bits, as inflate_sync.h has them; any two would do)


def expected(start, endp, have, flg, first, stop_bits):
    pe = [first] + list(endp[:N - 1])                     # the ends shifted up one lane, `first` entering at lane 0
    b = N
    for t in range(N):
        if not (have[t] and (t == 0 or start[t] == pe[t])):
            b = t
            break
    stop = N
    for t in range(b):                                    # a stop at or behind the break does not count
        if flg[t] & stop_bits:
            stop = t
            break
    return b, stop, stop + 1 if stop < N else b


def chain(first=5, step=544):
    """A round whose chain holds over all 64 lanes: every lane decoded from where its left neighbour ended."""
    endp = [first + step * (t + 1) + (t * 7) % 13 for t in range(N)]
    start = [first] + endp[:N - 1]
    return start, endp, [True] * N, [0] * N


def check(start, endp, have, flg, first, stop_bits, want=None):
    got = E.chain_check(start, endp, have, flg, first, stop_bits)
    assert got == expected(start, endp, have, flg, first, stop_bits)
    if want is not None:
        assert got == want


def test_chain_holds_over_all_lanes():
    start, endp, have, flg = chain()
    check(start, endp, have, flg, 5, EOB, (64, 64, 64))
    start[0] = 999                                        # lane 0's start is the round's: it is not compared with anything
    check(start, endp, have, flg, 5, EOB, (64, 64, 64))


@pytest.mark.parametrize("k", [1, 31, 32, 63])
def test_first_break_by_a_wrong_start(k):
    start, endp, have, flg = chain()
    start[k] += 1
    if k + 5 < N:
        start[k + 5] += 1                                 # a second break behind the first changes nothing
    check(start, endp, have, flg, 5, EOB, (k, 64, k))


@pytest.mark.parametrize("k", [0, 1, 31, 32, 63])
def test_first_break_by_a_lane_not_decoded(k):
    start, endp, have, flg = chain()
    have[k] = False                                       # (k == 0: lane 0 without `have`, the state after the walk)
    check(start, endp, have, flg, 5, EOB, (k, 64, k))


def test_nothing_decoded_yet():
    start, endp, _, flg = chain()
    check(start, endp, [False] * N, flg, 5, EOB, (0, 64, 0))


def test_kposfail_end_breaks_the_chain_behind_it():
    start, endp, have, flg = chain()
    endp[9] = 0xFFFFFFFF
    check(start, endp, have, flg, 5, EOB, (10, 64, 10))


@pytest.mark.parametrize("stop,want", [(19, (20, 19, 20)),    # in front of the break: the round ends with the stopped lane
                                       (0, (20, 0, 1)),
                                       (20, (20, 64, 20)),    # at the break: that lane is not on the chain, its stop does not count
                                       (21, (20, 64, 20)),    # behind the break
                                       (63, (20, 64, 20))])
def test_stop_against_a_break_at_lane_20(stop, want):
    start, endp, have, flg = chain()
    start[20] -= 3
    flg[stop] = EOB
    check(start, endp, have, flg, 5, EOB, want)


@pytest.mark.parametrize("stop", [0, 63])
def test_stop_at_the_ends_of_a_whole_chain(stop):
    start, endp, have, flg = chain()
    flg[stop] = EOB
    flg[63] |= EOB                                        # (a later stop behind the first changes nothing)
    check(start, endp, have, flg, 5, EOB, (64, stop, stop + 1))


def test_stop_bits_select_the_flags_that_stop():
    start, endp, have, flg = chain()
    flg[7] = FAIL
    flg[12] = EOB | FAIL
    check(start, endp, have, flg, 5, EOB, (64, 12, 13))          # one flag of the two that lane 12 has set; lane 7's is not asked for
    check(start, endp, have, flg, 5, FAIL, (64, 7, 8))
    check(start, endp, have, flg, 5, 4, (64, 64, 64))            # a bit nobody has set
    check(start, endp, have, flg, 5, 0xFFFFFFFF, (64, 7, 8))     # all ones (the LZ4 parse): any flag stops
    check(start, endp, have, flg, 5, 0, (64, 64, 64))


def random_case(rnd):
    first = rnd.randrange(32)
    start, endp, have, flg = chain(first, rnd.choice([1, 128, 544]))
    for _ in range(rnd.choice([0, 0, 1, 1, 2, 5])):       # breaks
        k = rnd.randrange(N)
        if rnd.random() < 0.5:
            have[k] = False
        else:
            start[k] ^= 1 << rnd.randrange(32)
    for _ in range(rnd.choice([0, 0, 1, 1, 2, 5])):       # flags
        flg[rnd.randrange(N)] = rnd.choice([1, 2, 3, 4, 8, 10, 0x80000000])
    if rnd.random() < 0.1:
        endp[rnd.randrange(N)] = 0xFFFFFFFF
    return start, endp, have, flg, first, rnd.choice([1, 1, 2, 3, 8, 0xFFFFFFFF])


def test_random_rounds_in_every_lane_order():
    rnd = random.Random(20240611)
    cases = [random_case(rnd) for _ in range(300)]
    try:
        for order in (0, 1, 2):
            E.set_order(order)
            for c in cases:
                check(*c)
    finally:
        E.set_order(0)
