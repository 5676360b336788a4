"""The host emulation built twice from tests/host_emu/emu_deflate_pairs.cpp: `pairs` as the sources are, `plain` with
-DSWC_SYNC_NO_PAIRS=1 (csrc/inflate_sync.h: the table entry format without PAIR entries).  Both hold every driver of libswc_emu.so
and two entry points of their own: the direct tables of a set of code lengths, and phase 1 of one stream with what it leaves in
the workspace.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import threading

import _emu

_DIR = _emu._DIR
_LIBS = {"pairs": (os.path.join(_DIR, "libswc_emu_pairs.so"), ()), "plain": (os.path.join(_DIR, "libswc_emu_nopairs.so"), ("-DSWC_SYNC_NO_PAIRS=1",))}


def _build_one(path, defines):
    tmp = "%s.%d.tmp" % (path, os.getpid())
    _emu._compile(tmp, "emu_deflate_pairs.cpp", ("-O2", "-g"), ("-fPIC", "-shared") + tuple(defines))
    os.replace(tmp, path)


def build():
    srcs = [os.path.join(_DIR, f) for f in os.listdir(_DIR) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(_emu._CSRC, f) for f in os.listdir(_emu._CSRC) if f.endswith(".h")]
    newest = max(os.path.getmtime(s) for s in srcs)
    todo = [v for v in _LIBS.values() if not os.path.exists(v[0]) or os.path.getmtime(v[0]) < newest]
    th = [threading.Thread(target=_build_one, args=v) for v in todo]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for path, _ in todo:
        assert os.path.exists(path), "the emulation did not build: " + path


build()
pairs = C.CDLL(_LIBS["pairs"][0])
plain = C.CDLL(_LIBS["plain"][0])
assert pairs.emu_pairs_enabled() == 1 and plain.emu_pairs_enabled() == 0
LIT_BITS = pairs.emu_pairs_lit_bits()
DIST_BITS = 8


def set_order(order):
    for lib in (pairs, plain):
        lib.emu_set_order(C.c_int(order))


def set_team(on):
    for lib in (pairs, plain):
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


def inflate(lib, inputs, caps):
    """Both phases, stream by stream: list of (status, bytes, in_consumed, out_len)."""
    return _emu.run_batch("emu_inflate_sync", inputs, caps, lib=lib)
