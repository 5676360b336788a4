"""Where the blocks of a .bz2 file start: what finding them on the device ("bzip2_scan_bytes", csrc/bzip2_scan.h)
costs and gains against the host scan, end to end on the host clock and for the index alone.

Two files, built here with bz2 at level 9 from BLOCKS chunks of 899,000 bytes of P-text (DISTINCT different ones, repeated):

    one stream        the chunks compressed as ONE stream of about BLOCKS blocks     -> swc_bzip2_decompress
    many streams      every chunk a stream of its own, back to back                  -> swc_bzip2_multi_decompress

    (a) each call with the knob at 0 and at 1: one discarded warm-up call and STEPS timed calls, mean and sigma of the host clock
        around the call in ms, and what one call issues (swc_stat)
    (b) swc_batch_bzip2_index alone on the file in HBM: HIP events around LOOP calls in a row (a single call of a tenth of a
        millisecond would measure the events and the launches as much as the kernels), ms per call, GB/s of the buffer -- and on
        268,435,456 bytes (the file of many streams repeated): what the kernels do once every SIMD has waves to choose from
    (c) swc_index_blocks kind 5 -- the host scan as it stands -- on the same bytes, by the host clock

With a library from before the knob, (a) has its knob-0 rows only and (b) is left out: the run of the parent commit's build that goes
into the file beside this one's.

    python tools/exp_bzip2_scan.py [STEPS] [--blocks N] [--distinct N] [--knob0-only] [--out FILE.txt]

--knob0-only: the rows a library from before the knob has, and nothing else -- the same process as the parent's, for comparing the two."""
import bz2
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP = 50   # index calls between two events in (b)


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        if name in argv:
            v = argv[argv.index(name) + 1]
            del argv[argv.index(name):argv.index(name) + 2]
            return v
        return default
    out_path, blocks, distinct = opt("--out", None), int(opt("--blocks", 256)), int(opt("--distinct", 16))
    knob0_only = "--knob0-only" in argv
    if knob0_only:
        argv.remove("--knob0-only")
    steps = int(argv[0]) if argv else 10
    if not any(os.path.isdir(os.path.join(p, "swcompression_amd")) for p in sys.path if p):
        sys.path.insert(0, ROOT)
    import torch
    import swcompression_amd as swc
    from swcompression_amd import _lib, corpus
    lib = _lib.load()
    assert swc.device_available(), "no usable gfx950 device"
    has_key = lib.swc_set_tuning(b"bzip2_scan_bytes", 0) == 0 and not knob0_only      # (a library from before the knob: the knob-0 rows only)

    distinct = min(distinct, blocks)
    chunks = [corpus.p_text(899000, 0xB21 + i) for i in range(distinct)]
    order = [chunks[i % distinct] for i in range(blocks)]
    total = 899000 * blocks
    one = bz2.compress(b"".join(order), 9)
    each = [bz2.compress(c, 9) for c in chunks]
    many = b"".join(each[i % distinct] for i in range(blocks))
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    keys = (b"launches", b"units", b"bzip2_scan_files", b"bzip2_scan_marks")

    def single(data):
        out, n, used = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_size_t()
        st = lib.swc_bzip2_decompress(data, len(data), C.byref(out), C.byref(n), C.byref(used))
        ok = st == 0 and n.value == total and used.value == len(data) and C.string_at(out, 64) == order[0][:64]
        lib.swc_free(out)
        return ok

    def multi(data):
        out, n, sizes, cnt = C.POINTER(C.c_uint8)(), C.c_size_t(), C.POINTER(C.c_size_t)(), C.c_size_t()
        st = lib.swc_bzip2_multi_decompress(data, len(data), C.byref(out), C.byref(n), C.byref(sizes), C.byref(cnt))
        ok = st == 0 and n.value == total and cnt.value == blocks and sizes[blocks - 1] == 899000
        lib.swc_free(out)
        lib.swc_free(sizes)
        return ok

    def row(name, call, data, k):
        if has_key:
            assert lib.swc_set_tuning(b"bzip2_scan_bytes", k) == 0
        try:
            assert call(data)      # warm-up, discarded
            at = [lib.swc_stat(s) for s in keys]
            ms = []
            for _ in range(steps):
                t0 = time.perf_counter()
                ok = call(data)
                ms.append((time.perf_counter() - t0) * 1e3)
                assert ok
            l, u, f, m = [max(lib.swc_stat(s) - a, 0) // steps for s, a in zip(keys, at)]
        finally:
            if has_key:
                lib.swc_set_tuning(b"bzip2_scan_bytes", 0)
        mean, sigma = statistics.mean(ms), statistics.pstdev(ms)
        say("%-44s %9.2f +- %-7.2f ms  %6.2f GiB/s of output   %d launches, %d units, %d files and %d block marks from the device per call"
            % (name, mean, sigma, total / (mean / 1e3) / 2**30, l, u, f, m))
        return mean

    say("bzip2, %d chunks of 899,000 bytes of P-text (%d distinct) at level 9: one stream of %d bytes, %d streams of %d bytes together -> %d; %s"
        % (blocks, distinct, len(one), blocks, len(many), total, torch.cuda.get_device_name(0)))
    say("(a) %d timed calls after one discarded warm-up call each; mean +- sigma of the host clock around the call (host buffers both ways)" % steps)
    for name, call, data in (("swc_bzip2_decompress, one stream", single, one), ("swc_bzip2_multi_decompress, many streams", multi, many)):
        a0 = row("%s, knob 0" % name, call, data, 0)
        if has_key:
            a1 = row("%s, knob 1" % name, call, data, 1)
            say("    knob 1 takes %.3f of the time of knob 0" % (a1 / a0))

    big = (many * (268435456 // len(many) + 1))[:268435456]
    for name, data in (("one stream", one), ("many streams", many), ("many streams repeated", big)):
        n_bytes = len(data)
        n_found = C.c_size_t()
        ms = []
        for _ in range(steps + 1):
            t0 = time.perf_counter()
            assert lib.swc_index_blocks(5, data, n_bytes, None, 0, C.byref(n_found)) == 0
            ms.append((time.perf_counter() - t0) * 1e3)
        host_mean, host_sigma = statistics.mean(ms[1:]), statistics.pstdev(ms[1:])
        say("(c) swc_index_blocks kind 5 (the host scan), %s, %d bytes, %d block magics: %.3f +- %.3f ms (host clock), %.2f GB/s of the buffer"
            % (name, n_bytes, n_found.value, host_mean, host_sigma, n_bytes / host_mean / 1e6))
        if not has_key:
            continue
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        cap = max(4096, n_bytes // 4096)
        ws = torch.empty(lib.swc_bzip2_index_workspace_bytes(n_bytes, cap), dtype=torch.uint8, device="cuda")
        refs = torch.empty((cap, 4), dtype=torch.int64, device="cuda")
        n = torch.zeros(1, dtype=torch.int64, device="cuda")
        opts = _lib.SwcBatchOpts(-1, torch.cuda.current_stream().cuda_stream, 0, 0)

        def call():
            assert lib.swc_batch_bzip2_index(src.data_ptr(), n_bytes, refs.data_ptr(), cap, n.data_ptr(), ws.data_ptr(), int(ws.numel()), C.byref(opts)) == 0
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LOOP):
                call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / LOOP)
        mean, sigma = statistics.mean(ms), statistics.pstdev(ms)
        say("(b) swc_batch_bzip2_index alone, %s, %d bytes in HBM, %d marks: %.3f +- %.3f ms per call (HIP events around %d calls in a row), "
            "%.0f GB/s of the buffer; (c) takes %.0f times as long" % (name, n_bytes, int(n.item()), mean, sigma, LOOP, n_bytes / mean / 1e6, host_mean / mean))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
