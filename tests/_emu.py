"""ctypes binding of tests/host_emu/libswc_emu.so -- the device code compiled for the host: the one library of the CPU tier (every
entry point is in it), its variants under a -DSWC_SYNC_* switch of csrc/inflate_sync.h (libswc_emu.<tag>.so: one line of VARIANTS
each), the one build recipe, the one rule for rebuilding and the one way to run a stand-alone sanitizer program.  The _emu_*.py
modules are layers over `lib`.  TEST INFRASTRUCTURE ONLY (see tests/host_emu/emu.cpp)."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "host_emu")
_CSRC = os.path.join(os.path.dirname(_HERE), "swcompression_amd", "csrc")

# tag -> (defines, what emu_pairs_enabled() says, what emu_sync_follow() says); None: the sources as they ship
VARIANTS = {None: ((), 1, 1),
            "nopairs": (("-DSWC_SYNC_NO_PAIRS=1",), 0, 1),
            "nofollow": (("-DSWC_SYNC_NO_FOLLOW=1",), 1, 0),
            "follow_held": (("-DSWC_SYNC_FOLLOW_HELD=1",), 1, 2)}


class Job(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_len", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_uint64),
                ("out_len", C.c_uint64), ("in_consumed", C.c_uint64), ("status", C.c_int32), ("aux", C.c_int32),
                ("dict", C.c_void_p), ("dict_len", C.c_uint64)]


def _compile(out, src, opt, how):
    subprocess.run(["g++"] + list(opt) + ["-std=c++17", "-DSWC_HOST_EMULATION"] + list(how) +
                   ["-Wno-unknown-pragmas", "-pthread", "-o", out, os.path.join(_DIR, src)], check=True)


def compile_lib(out, opt=("-O2", "-g"), defines=()):
    """The one recipe of the emulation library (emu.cpp includes the other sources); the ASAN tests pass their own optimisation and
    sanitizer flags."""
    _compile(out, "emu.cpp", opt, ("-fPIC", "-shared") + tuple(defines))


SANITIZED = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def compile_program(out, src, define, opt=SANITIZED):
    """A source of host_emu that has a main of its own behind -D`define`, as a stand-alone program: by default with the address and
    undefined-behaviour sanitizers.  Run as a program, never loaded into python."""
    _compile(out, src, opt, ("-D" + define,))


def run_program(tmp_path, src, define, case_bytes, opt=SANITIZED, timeout=600):
    """compile_program, then the program once on a file of `case_bytes`: asserts that it ends with status 0, returns what it printed."""
    exe, cases = str(tmp_path / src[:-4]), str(tmp_path / "cases.bin")
    compile_program(exe, src, define, opt)
    with open(cases, "wb") as f:
        f.write(case_bytes)
    p = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, errors="replace", timeout=timeout,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


def _path(tag):
    return os.path.join(_DIR, "libswc_emu.so" if tag is None else "libswc_emu.%s.so" % tag)


_newest = None   # the newest source's time: scanned once per process


def _stale(path):
    """The one rule: a library is rebuilt when any source of host_emu or any header of csrc is newer than it."""
    global _newest
    if _newest is None:
        srcs = [os.path.join(_DIR, f) for f in os.listdir(_DIR) if f.endswith((".cpp", ".h"))]
        srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")]
        _newest = max(os.path.getmtime(s) for s in srcs)
    return not os.path.exists(path) or os.path.getmtime(path) < _newest


def _build_one(tag):
    tmp = "%s.%d.tmp" % (_path(tag), os.getpid())
    compile_lib(tmp, defines=VARIANTS[tag][0])
    os.replace(tmp, _path(tag))   # (a process that has the old file loaded keeps it)


def build(force=False, tags=tuple(VARIANTS)):
    """Builds, in parallel, those of `tags` that are stale -- with `force`, all of them."""
    todo = [t for t in tags if force or _stale(_path(t))]
    with ThreadPoolExecutor(max(len(todo), 1)) as ex:
        list(ex.map(_build_one, todo))


_loaded = {}


def load(tag=None):
    """The library of a tag of VARIANTS, built if stale and held to what it says of itself."""
    if tag not in _loaded:
        build(tags=(tag,))
        so = C.CDLL(_path(tag))
        says = (so.emu_pairs_enabled(), so.emu_sync_follow())
        assert says == VARIANTS[tag][1:], "%s says pairs %d, follow %d of itself" % ((_path(tag),) + says)
        _loaded[tag] = so
    return _loaded[tag]


lib = load()


def set_order(order):
    """Thread order of the emulated SIMT regions (csrc/simt.h) in every library loaded so far: 0 forward, 1 reverse, 2 shuffled."""
    for so in _loaded.values():
        so.emu_set_order(C.c_int(order))


class Guarded:
    """`n` bytes that start `residue` bytes past an `align`-byte boundary, with at least `guard` bytes of `fill` on both sides:
    .addr is their address."""

    def __init__(self, n, residue=0, align=16, guard=16, fill=0xA5, data=b""):
        self._buf = C.create_string_buffer(align + guard + residue + n + guard)
        C.memset(self._buf, fill, len(self._buf))
        base = C.addressof(self._buf)
        self.addr = base + (-base) % align + guard + residue
        self.n = n
        self._fill = bytes([fill])
        C.memmove(self.addr, bytes(data), len(data))

    def read(self, lo=0, hi=None):
        return C.string_at(self.addr + lo, (self.n if hi is None else hi) - lo)

    def check(self, what="", used=None):
        """Asserts that every byte in front of the n bytes and every byte behind them -- behind the first `used` of them, where given --
        still holds the fill value."""
        base = C.addressof(self._buf)
        front, end = self.addr - base, self.addr + (self.n if used is None else used)
        back = base + len(self._buf) - end
        assert C.string_at(base, front) == self._fill * front, "guard bytes in front overwritten (%s)" % what
        assert C.string_at(end, back) == self._fill * back, "guard bytes behind overwritten (%s)" % what


def run_batch(fn_name, inputs, caps, aux=None, dicts=None, extra=None, fn_args=(), dict_ptr_values=None, misalign=0, lib=None,
              in_misalign=None, exact=False):
    """inputs: list[bytes]; caps: list[int].  Returns list of (status, out_bytes, in_consumed, out_len).
    misalign: the output buffers start that many bytes past a 16-byte boundary, 16 guard bytes on either side.  lib: another build
    of the library (ASAN).  in_misalign (not None): the inputs -- and the dictionaries, seven residues further -- lie in guarded
    buffers of their own that many bytes past a 16-byte boundary, and are checked unchanged afterwards.  exact: the bytes of an output
    buffer behind the first min(out_len, capacity) count as guard bytes too -- nothing may be written there."""
    n = len(inputs)
    jobs = (Job * n)()
    keep, outs, ins = [], [], []
    for i, (data, cap) in enumerate(zip(inputs, caps)):
        if in_misalign is None:
            ib = C.create_string_buffer(bytes(data), max(len(data), 1))
            keep.append(ib)
        else:
            ins.append((Guarded(len(data), in_misalign, data=data), bytes(data), "input of job %d" % i))
        outs.append(Guarded(cap, misalign))
        jobs[i].in_ = C.addressof(ib) if in_misalign is None else ins[-1][0].addr
        jobs[i].in_len = len(data)
        jobs[i].out = outs[i].addr
        jobs[i].out_cap = cap
        jobs[i].aux = 0 if aux is None else aux[i]
        if dicts is not None and dicts[i] is not None:
            if in_misalign is None:
                db = C.create_string_buffer(bytes(dicts[i]), max(len(dicts[i]), 1))
                keep.append(db)
                jobs[i].dict = C.addressof(db)
            else:
                ins.append((Guarded(len(dicts[i]), (in_misalign + 7) % 16, data=dicts[i]), bytes(dicts[i]), "dictionary of job %d" % i))
                jobs[i].dict = ins[-1][0].addr
            jobs[i].dict_len = len(dicts[i])
        if extra is not None:
            jobs[i].dict_len = extra[i]
        if dict_ptr_values is not None:
            jobs[i].dict = dict_ptr_values[i]
    getattr(lib or globals()["lib"], fn_name)(jobs, C.c_size_t(n), *fn_args)
    res = []
    for buf, data, what in ins:
        buf.check(what)
        assert buf.read() == data, "%s changed" % what
    for i in range(n):
        outs[i].check("job %d" % i, used=min(jobs[i].out_len, caps[i]) if exact else None)
        res.append((jobs[i].status, outs[i].read(0, min(jobs[i].out_len, caps[i])), jobs[i].in_consumed, jobs[i].out_len))
    return res


def inflate(inputs, caps, misalign=0, in_misalign=None):
    """Deflate: inflate_sync.h (one stream per wavefront, 64 sub-chunks at once) + lz_resolve.h."""
    return run_batch("emu_inflate_sync", inputs, caps, misalign=misalign, in_misalign=in_misalign)


def lz4_block(inputs, caps, dicts=None, misalign=0, in_misalign=None, aux=None, exact=False):
    """aux: the swc_lz4_aux bits of every job (SWC_LZ4_STORED = 2: `in` is copied)."""
    return run_batch("emu_lz4_block", inputs, caps, aux=aux, dicts=dicts, misalign=misalign, in_misalign=in_misalign, exact=exact)


LZMA_MODE = 0   # 0: literal coders in LDS / cell-by-cell spill (kernel without a workspace); 1: LDS as a cache of four coders


def lzma2(inputs, caps, dict_bytes, mode=None, **place):
    return run_batch("emu_lzma_mode", inputs, caps, aux=dict_bytes, fn_args=(C.c_int(1), C.c_int(LZMA_MODE if mode is None else mode)), **place)


def lzma(inputs, caps, props, dict_sizes, sizes, mode=None, **place):
    """props: list of (lc, lp, pb); sizes: declared uncompressed size or -1.  place: misalign / in_misalign of run_batch."""
    aux = [lc | (lp << 8) | (pb << 16) for lc, lp, pb in props]
    extra = [s & 0xFFFFFFFFFFFFFFFF for s in sizes]
    return run_batch("emu_lzma_mode", inputs, caps, aux=aux, extra=extra, fn_args=(C.c_int(0), C.c_int(LZMA_MODE if mode is None else mode)),
                     dict_ptr_values=dict_sizes, **place)


_bzip2_team = None


def set_bzip2_team(mode):
    """None: stage 3a inside the block's own wavefront (bzip2_block.h); (start_team, one_thread): stage 3a as kernels of its own
    (bzip2_team.h) -- the team whose thread goes first, and whether that thread alone draws all teams' tickets."""
    global _bzip2_team
    _bzip2_team = mode


def bzip2_block(streams, body_bits, crcs, caps, lcap=1000000, **place):
    """One bzip2 block per job: `streams[i]` is the whole stream, body_bits[i] the bit offset of the block body."""
    if _bzip2_team is not None:
        return run_batch("emu_bzip2_block_team", streams, caps, extra=body_bits, dict_ptr_values=crcs,
                         fn_args=(C.c_size_t(lcap), C.c_int(_bzip2_team[0]), C.c_int(_bzip2_team[1])), **place)
    return run_batch("emu_bzip2_block", streams, caps, extra=body_bits, dict_ptr_values=crcs, fn_args=(C.c_size_t(lcap),), **place)


lib.emu_checksum.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
lib.emu_checksum.restype = C.c_uint64


def checksum(kind, data, misalign=0):
    """kind: 1 crc32, 2 adler32, 3 crc64, 4 bzip2crc32, 5 xxh32 (swc_checksum of include/swc_hip.h).  The data are
    placed `misalign` bytes past a 64-byte boundary."""
    buf = Guarded(len(data), misalign, align=64, data=data)
    got = lib.emu_checksum(kind, buf.addr, buf.n)
    buf.check("checksum %d" % kind)
    return got


lib.emu_crc32_wave.argtypes = [C.c_void_p, C.c_size_t]
lib.emu_crc32_wave.restype = C.c_uint32


def crc32_wave(data, misalign=0):
    """CRC-32 by the wave-per-stream code of the device (crc32_wave.h), the data `misalign` bytes past a 64-byte boundary."""
    buf = Guarded(len(data), misalign, align=64, data=data)
    got = lib.emu_crc32_wave(buf.addr, buf.n)
    buf.check("crc32_wave")
    return got


lib.emu_chain_check.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.c_uint32,
                                C.c_uint32, C.POINTER(C.c_uint32)]
lib.emu_chain_check.restype = None


def chain_check(start, endp, have, flg, first, stop_bits):
    """The chain check of a sub-chunk round (sync_round.h) over 64 lanes: returns (b, E, nv)."""
    u32 = C.c_uint32 * 64
    out = (C.c_uint32 * 3)()
    lib.emu_chain_check(u32(*start), u32(*endp), (C.c_uint8 * 64)(*[1 if h else 0 for h in have]), u32(*flg), first, stop_bits, out)
    return tuple(out)


lib.emu_delta.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_uint]
lib.emu_delta.restype = None


def delta(data, distance, in_place=False):
    """DeltaFilter.decode by the device group code (256 host threads).  distance as the reference passes it (0..255)."""
    data = bytes(data)
    if in_place:
        buf = C.create_string_buffer(data, max(len(data), 1))
        lib.emu_delta(C.cast(buf, C.c_char_p), C.cast(buf, C.c_void_p), len(data), distance)
        return buf.raw[:len(data)]
    out = C.create_string_buffer(max(len(data), 1))
    lib.emu_delta(data, C.cast(out, C.c_void_p), len(data), distance)
    return out.raw[:len(data)]


def delta_placed(data, distance, in_misalign, misalign, in_place=False):
    """delta() with the input and the output in guarded buffers at those residues mod 16 (in place: one buffer, at `misalign`); the
    guards are checked, and the input where it is not the output."""
    data = bytes(data)
    out = Guarded(len(data), misalign, data=data if in_place else b"")
    src = out if in_place else Guarded(len(data), in_misalign, data=data)
    lib.emu_delta(C.c_char_p(src.addr), C.c_void_p(out.addr), len(data), distance)
    out.check("delta output")
    if not in_place:
        src.check("delta input")
        assert src.read() == data, "delta input changed"
    return out.read()


def lz4_compress(blocks, prefixes=None, caps=None, **place):
    """LZ4 block compression (lz4_comp.h): returns list of (status, compressed bytes, in_consumed, out_len)."""
    prefixes = prefixes or [b""] * len(blocks)
    ins = [bytes(p) + bytes(b) for p, b in zip(prefixes, blocks)]
    caps = caps or [len(b) + len(b) // 255 + 16 for b in blocks]
    return run_batch("emu_lz4_compress", ins, caps, extra=[len(p) for p in prefixes], **place)


def deflate_compress(bufs, caps=None, aux=None, **place):
    """Deflate compression (deflate_comp.h): returns list of (status, compressed bytes, in_consumed, out_len).  aux[i] & 1: unit i
    is a segment of a longer stream (BFINAL clear, an empty stored block behind its block)."""
    caps = caps or [len(b) + len(b) // 8 + 32 for b in bufs]
    return run_batch("emu_deflate_compress", [bytes(b) for b in bufs], caps, aux=aux, **place)


def bzip2_compress(data, block_size=1):
    """BZip2 compression (bzip2_comp.h) with the emulation's executor: returns (status, stream bytes)."""
    data = bytes(data)
    cap = len(data) + len(data) // 2 + 4096
    ob = C.create_string_buffer(cap)
    n = C.c_size_t(0)
    lib.emu_bzip2_compress.restype = C.c_int
    st = lib.emu_bzip2_compress(C.c_char_p(data), C.c_size_t(len(data)), C.c_int(block_size), ob, C.c_size_t(cap), C.byref(n))
    assert n.value <= cap
    return st, ob.raw[:n.value]
