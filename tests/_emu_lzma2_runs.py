"""LZMA2 streams cut at their dictionary resets (include/swc_hip.h: SWC_LZMA2_OPEN, swc_index_blocks kind 8) on the host emulation:
a thin layer over _emu that fills the jobs itself -- the units lie IN PLACE in one buffer, their outputs back to back in another --
and reads `aux` back.  Also the stream recipes and the acceptance rule the CPU and the GPU tier share.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import lzma as _pylzma
import struct

import _emu
import _lzma_build as B
from _emu import Job

OPEN = 0x100
GUARD = 16
RECIPE_DICT_BYTE = 8   # 64 KiB: what recipe() hands to liblzma
SHAPES = [(0, 4, 4), (3, 0, 2), (1, 3, 4), (4, 0, 0)]


def recipe(parts, shape=(3, 0, 2)):
    """One LZMA2 stream (chunks only, no dictionary-size byte) of independently compressed parts: liblzma's raw LZMA2 of every part
    without its end marker, one end marker behind the last.  Every part opens with a chunk that resets dictionary, state and
    properties (0xE0, tiny incompressible parts: a stored 0x01).  Decodes to the concatenation of the parts."""
    lc, lp, pb = shape
    f = [{"id": _pylzma.FILTER_LZMA2, "lc": lc, "lp": lp, "pb": pb, "dict_size": 1 << 16}]
    out = b""
    for p in parts:
        z = _pylzma.compress(bytes(p), format=_pylzma.FORMAT_RAW, filters=f)
        assert z[-1] == 0 and (z[0] >= 0xE0 or z[0] == 1)
        out += z[:-1]
    return out + b"\0"


def text(n, seed):
    """Compressible bytes, a function of (n, seed) alone."""
    import random
    rnd = random.Random(0x12A2 + seed)
    words = [bytes(rnd.choice(b"etaoinshrdlu") for _ in range(rnd.randrange(2, 9))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + (b" " if rnd.random() < 0.9 else b".\n")
    return bytes(out[:n])


def aligned_match_behind_reset():
    """_lzma_build._match_behind_reset with its reset at an output position that is a multiple of 16 -- a cut of kind 8: the match
    behind it reaches in front of the reset, legal in the stream (LZMADecoder.swift:269,297), a failure in the unit."""
    b = B._new("lzma2", (3, 0, 2), None)
    for i in range(112):
        b.literal((i * 3) & 0xFF)
    b.chunk(0xE0, (3, 0, 2))
    b.literal(1)
    b.match(60, 30)
    b.literal(2)
    return b.case("match-reaching-behind-a-dictionary-reset-at-112")


def aligned_stored_resets():
    """Streams whose model goes on behind a stored chunk that resets the dictionary AT a position that is a multiple of 16 -- where
    only the look-ahead of kind 8 forbids the cut: 0x01 then 0x80, 0x01 then 0xA0 (the properties are not the defaults, so a unit
    that began at the stored chunk would build the wrong model), 0x01 then 0x02 then 0x80.  Behind that, at another multiple of 16,
    a 0xE0 chunk: the one cut of the stream.  [(case, output position of the stored reset)]"""
    import random
    out = []
    for k, (name, second_stored, control) in enumerate((("0x80", False, 0x80), ("0xA0", False, 0xA0), ("0x02-then-0x80", True, 0x80))):
        rnd = random.Random(0x0180 + k)
        b = B._new("lzma2", (1, 2, 1), None)
        for _ in range(100):
            B._trained_literal(b, rnd)
        b.match(5, 12)
        at = len(b.out)
        assert at % 16 == 0
        b.stored(bytes([0xF3, 0x5A, 0xC4, 0x3D, 0xE1, 0x96, 0x0F, 0x78] * 2), True)
        if second_stored:
            b.stored(b"\x21\x43\x65\x87\xA9\xCB\xED", False)
        b.chunk(control)
        b.literal(0x5B)
        b.match(7, 12)                       # source: stored bytes, overlapping
        for _ in range(120):
            B.random_packet(b, rnd, False)
        while len(b.out) % 16:
            b.literal(rnd.randrange(256))
        b.chunk(0xE0, (3, 0, 2))
        for _ in range(60):
            B._trained_literal(b, rnd)
        c = b.case("aligned-stored-reset-then-" + name)
        assert c.status == 0
        out.append((c, at))
    return out


def run_jobs(buffer, units, mode):
    """One emulated launch of LZMA2 jobs that lie in place in `buffer` (bytes: read only through the jobs).  units: list of
    (offset, in_len, out_cap, aux).  The outputs lie back to back in one buffer with GUARD bytes of 0xA5 around it; asserts that the
    guards and every byte behind what a unit produced, up to the next unit's first byte, are intact and that `buffer` is unchanged.
    Returns per job (status, bytes, in_consumed, out_len, aux)."""
    n = len(units)
    ib = C.create_string_buffer(bytes(buffer), max(len(buffer), 1))
    total = sum(u[2] for u in units)
    ob = _emu.Guarded(total, 0, guard=GUARD)
    jobs = (Job * n)()
    at = []
    for i, (off, ln, cap, aux) in enumerate(units):
        assert off + ln <= len(buffer)
        at.append(sum(u[2] for u in units[:i]))
        jobs[i].in_ = C.addressof(ib) + off
        jobs[i].in_len = ln
        jobs[i].out = ob.addr + at[i]
        jobs[i].out_cap = cap
        jobs[i].aux = aux
        jobs[i].status = 902
    _emu.lib.emu_lzma_mode(jobs, C.c_size_t(n), C.c_int(1), C.c_int(mode))
    assert ib.raw[:len(buffer)] == bytes(buffer), "the input changed"
    ob.check("the outputs of the launch")
    res = []
    for i, (off, ln, cap, aux) in enumerate(units):
        k = min(jobs[i].out_len, cap)
        assert ob.read(at[i] + k, at[i] + cap) == b"\xA5" * (cap - k), "job %d wrote behind what it produced" % i
        res.append((jobs[i].status, ob.read(at[i], at[i] + k), jobs[i].in_consumed, jobs[i].out_len, jobs[i].aux))
    return res


def accept(refs, res):
    """The acceptance rule (include/swc_hip.h, swc_lzma2_aux) over the units kind 8 listed (`refs`: offset, comp_len, uncomp_len, aux --
    offsets as the jobs got them) and what their jobs left (`res`: status, bytes, in_consumed, out_len, aux).  Returns None, or
    (joined output, in_consumed of the stream)."""
    for (off, comp, uncomp, _), (st, _, cons, out_len, aux) in list(zip(refs, res))[:-1]:
        if not (st == 0 and aux & OPEN and cons == comp and out_len == uncomp):
            return None
    if res[-1][0] != 0:
        return None
    return b"".join(r[1] for r in res), refs[-1][0] + res[-1][2]


def case_file(cases):
    """The bytes of the file the stand-alone program reads.  cases: list of (chunks, refs, consumed, plain), refs as accept() takes them."""
    out = bytearray(struct.pack("<I", len(cases)))
    for chunks, refs, consumed, plain in cases:
        out += struct.pack("<I", len(chunks)) + bytes(chunks) + struct.pack("<I", len(refs))
        for off, comp, uncomp, aux in refs:
            out += struct.pack("<IIII", off, comp, uncomp, aux)
        out += struct.pack("<II", consumed, len(plain)) + bytes(plain)
    return bytes(out)
