"""A file of plain gzip members through GzipArchive.multi_unarchive: what the device scan for members ("gzip_member_scan",
csrc/gzip_scan.h) gains, end to end on the host clock, and what the index kernels cost alone.

The payload is that of bench.py's bgzf_multi_unarchive line -- 4,096 members of 64 KiB of P-text, 512 distinct -- written as

    (a) plain members, key 0      corpus.gzip_member without the 'BC' field; the walk decodes member by member: the shipped path, and
                                  the only one a build without the key has
    (b) plain members, key 1      the same file: staged once, indexed on the device, every candidate decoded in one launch
    (c) BGZF                      the same chunks with the 'BC' field: BSIZE locates the members, one launch -- what a launch costs

Per row one discarded warm-up call and STEPS timed calls (one process, as bench.py does it): mean and sigma in ms, and what one call
issues (swc_stat).  Then swc_batch_gzip_index alone on a buffer of 268 MB in HBM (the plain file repeated): HIP events around the call.

    python tools/exp_gzip_members.py [STEPS] [--members N] [--out FILE.txt]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        if name in argv:
            v = argv[argv.index(name) + 1]
            del argv[argv.index(name):argv.index(name) + 2]
            return v
        return default
    out_path, members = opt("--out", None), int(opt("--members", 4096))
    steps = int(argv[0]) if argv else 10
    if not any(os.path.isdir(os.path.join(p, "swcompression_amd")) for p in sys.path if p):
        sys.path.insert(0, ROOT)
    import torch
    import swcompression_amd as swc
    from swcompression_amd import _lib, batch, corpus
    lib = _lib.load()
    assert swc.device_available(), "no usable gfx950 device"

    distinct = min(512, members)
    parts = [corpus.p_text(65536, 0x5C0DE + 2 + i) for i in range(distinct)]
    reps = members // distinct
    plain = b"".join([corpus.gzip_member(p) for p in parts] * reps)
    bgzf = b"".join([corpus.gzip_member(p, bgzf=True) for p in parts] * reps)
    total = 65536 * distinct * reps
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    has_key = lib.swc_set_tuning(b"gzip_member_scan", 0) == 0      # (a library from before the key: row (a) only)
    keys = (b"launches", b"units", b"gzip_scan_members", b"gzip_scan_walked")

    def row(name, data, k):
        if has_key:
            assert lib.swc_set_tuning(b"gzip_member_scan", k) == 0
        try:
            out = swc.GzipArchive.multi_unarchive(data)      # warm-up, discarded
            assert len(out) == distinct * reps and out[0] == parts[0] and out[-1] == parts[-1] and sum(len(o) for o in out) == total
            at = [lib.swc_stat(s) for s in keys]
            ms = []
            for _ in range(steps):
                t0 = time.perf_counter()
                out = swc.GzipArchive.multi_unarchive(data)
                ms.append((time.perf_counter() - t0) * 1e3)
                assert len(out) == distinct * reps and out[-1] == parts[-1]
            del out
            l, u, m, w = [max(lib.swc_stat(s) - a, 0) // steps for s, a in zip(keys, at)]
        finally:
            if has_key:
                lib.swc_set_tuning(b"gzip_member_scan", 0)
        mean, sigma = statistics.mean(ms), statistics.pstdev(ms)
        say("%-26s %10.2f +- %-8.2f ms  %7.2f GiB/s   %d launches, %d units, %d members from the scan, %d walked per call"
            % (name, mean, sigma, total / (mean / 1e3) / 2**30, l, u, m, w))
        return mean

    say("GzipArchive.multi_unarchive, %d members x 64 KiB of P-text (%d distinct): %d bytes as plain members, %d as BGZF -> %d; %s"
        % (distinct * reps, distinct, len(plain), len(bgzf), total, torch.cuda.get_device_name(0)))
    say("%d timed calls after one discarded warm-up call each; mean +- sigma of the host clock around the call (host buffers both ways, "
        "the Python list of bytes included)" % steps)
    a = row("(a) plain members, key 0", plain, 0)
    b = row("(b) plain members, key 1", plain, 1) if has_key else None
    c = row("(c) BGZF", bgzf, 0)
    if b is not None:
        say("(b) takes %.3f of the time of (a) and %.2f of the time of (c)" % (b / a, b / c))

    if has_key:
        n_bytes = 268435456
        host = (plain * (n_bytes // len(plain) + 1))[:n_bytes]
        src = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
        cap = max(4096, n_bytes // 256)
        ws = torch.empty(batch.gzip_index_workspace_bytes(n_bytes, cap), dtype=torch.uint8, device="cuda")
        refs = torch.empty((cap, 4), dtype=torch.int64, device="cuda")
        n = torch.zeros(1, dtype=torch.int64, device="cuda")
        opts = _lib.SwcBatchOpts(-1, torch.cuda.current_stream().cuda_stream, 0, 0)

        def call():
            assert lib.swc_batch_gzip_index(src.data_ptr(), n_bytes, refs.data_ptr(), cap, n.data_ptr(), ws.data_ptr(), int(ws.numel()), C.byref(opts)) == 0
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        mean, sigma = statistics.mean(ms), statistics.pstdev(ms)
        say("swc_batch_gzip_index alone, %d bytes in HBM (the plain file repeated), %d candidates: %.3f +- %.3f ms (HIP events), %.0f GB/s of the buffer, "
            "two passes over it" % (n_bytes, int(n.item()), mean, sigma, n_bytes / mean / 1e6))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
