"""Deflate phase 1 on the host emulation as it ships and in its differential builds (_emu.VARIANTS; csrc/inflate_sync.h): `plain`
with -DSWC_SYNC_NO_PAIRS=1 (the table entry format without PAIR entries), `single` with -DSWC_SYNC_NO_FOLLOW=1 (the provisional
decode with one code per step, as it was), `held` with -DSWC_SYNC_FOLLOW_HELD=1 (the follow-up literal's bits from the window the
step already holds: the form that is not shipped).  The entry points are those of tests/host_emu/emu_deflate_phase1.cpp: the direct
tables of a set of code lengths, and phase 1 of one stream with what it leaves in the workspace; the step counters of the emulated
decoder come with them.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import _emu

_emu.build()   # (whatever is stale, at once)
shipped = _emu.lib
plain = _emu.load("nopairs")
single = _emu.load("nofollow")
held = _emu.load("follow_held")
ALL = (shipped, plain, single, held)
LIT_BITS = shipped.emu_pairs_lit_bits()
DIST_BITS = 8

set_order = _emu.set_order


def set_team(on):
    for lib in ALL:
        lib.emu_set_deflate_team(C.c_int(on))


def tables(lib, lit_lengths, dist_lengths):
    """-> (the fast path takes the set, the direct lit/len entries, the direct distance entries)"""
    lens = bytes(lit_lengths) + bytes(dist_lengths)
    n = (1 << LIT_BITS) + (1 << DIST_BITS)
    lut = (C.c_uint32 * n)()
    fast = lib.emu_pairs_tables(lens, C.c_int(len(lit_lengths)), C.c_int(len(dist_lengths)), lut)
    return bool(fast), list(lut[:1 << LIT_BITS]), list(lut[1 << LIT_BITS:])


def phase1(lib, data, cap, aux=0, team=0):
    """Phase 1 of one stream: (status, out_len, in_consumed, aux, nrec, reach, nlit, records, literal stream)."""
    data = bytes(data)
    max_rec, max_lit = cap // 2 + 4096, cap + 4096
    res = (C.c_uint64 * 7)()
    recs = (C.c_uint32 * max_rec)()
    lits = C.create_string_buffer(max_lit)
    lib.emu_pairs_phase1(data, C.c_size_t(len(data)), C.c_size_t(cap), C.c_int(aux), C.c_int(team), res, recs, C.c_size_t(max_rec), lits, C.c_size_t(max_lit))
    st = C.c_int32(res[0] & 0xFFFFFFFF).value
    nrec, nlit = min(res[4], max_rec), min(res[6], max_lit)
    return (st, res[1], res[2], C.c_int32(res[3] & 0xFFFFFFFF).value, res[4], res[5], res[6], bytes(bytearray(recs)[:4 * nrec]), lits.raw[:nlit])


def counted(lib, data, cap, aux=0, team=0):
    """phase1, and what the emulated decoder counted meanwhile: (result, rounds committed, rounds abandoned, lanes decoded by the
    provisional pass, steps of the provisional pass)."""
    out = (C.c_uint64 * 8)()
    lib.emu_sync_stats(out, C.c_int(1))
    r = phase1(lib, data, cap, aux, team)
    lib.emu_sync_stats(out, C.c_int(1))
    return r, int(out[0]), int(out[1]), int(out[3]), int(out[5])


def inflate(lib, inputs, caps):
    """Both phases, stream by stream: list of (status, bytes, in_consumed, out_len)."""
    return _emu.run_batch("emu_inflate_sync", inputs, caps, lib=lib)
