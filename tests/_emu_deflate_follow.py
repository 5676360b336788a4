"""The host emulation built three times from tests/host_emu/emu_deflate_pairs.cpp: `follow` as the sources are, `single` with
-DSWC_SYNC_NO_FOLLOW=1 (csrc/inflate_sync.h: the provisional decode with one code per step, as it was), and `held` with
-DSWC_SYNC_FOLLOW_HELD=1 (the follow-up literal's bits from the window the step already holds: the form that is not shipped).
The entry points are those of _emu_deflate_pairs; the step counters of the emulated decoder come with them.  TEST INFRASTRUCTURE
ONLY."""
import ctypes as C
import os
import threading

import _emu

_DIR = _emu._DIR
_LIBS = {"follow": (os.path.join(_DIR, "libswc_emu_follow.so"), ()),
         "single": (os.path.join(_DIR, "libswc_emu_nofollow.so"), ("-DSWC_SYNC_NO_FOLLOW=1",)),
         "held": (os.path.join(_DIR, "libswc_emu_follow_held.so"), ("-DSWC_SYNC_FOLLOW_HELD=1",))}


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
follow = C.CDLL(_LIBS["follow"][0])
single = C.CDLL(_LIBS["single"][0])
held = C.CDLL(_LIBS["held"][0])
ALL = (follow, single, held)
LIT_BITS = follow.emu_pairs_lit_bits()


def set_order(order):
    for lib in ALL:
        lib.emu_set_order(C.c_int(order))


def set_team(on):
    for lib in ALL:
        lib.emu_set_deflate_team(C.c_int(on))


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
