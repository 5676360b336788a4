"""LZMA2 streams cut at their dictionary resets: what swc_lzma2_decompress costs, end to end on the host clock (every call ends
with a device synchronise and the copy of the result).

    16 runs, key 0           one stream of RUNS runs x KIB KiB of P-text, each run compressed on its own (a dictionary reset per run,
                             what a multi-threaded LZMA2 encoder writes), "lzma2_run_bytes" = 0: one job on one wavefront -- the shipped
                             path, and the only one a build without the key has
    16 runs, key 65536       the same stream cut into its runs: RUNS jobs in one launch
    1 run, key 0 / 65536     the same payload as ONE run: nothing to cut -- what the index walk costs

Per row one discarded warm-up call and STEPS timed calls: mean and sigma in ms, the launches, units and fallbacks one call issues
(swc_stat), the result compared with the payload.

A library from before the key -- swc_set_tuning refuses "lzma2_run_bytes" -- runs the rows with the key at 0, so the same file measures
the parent's build: SWC_LIB=<that build's libswc_hip.so> (the Python layer of these calls is the same), or that build's package
first on PYTHONPATH.

    python tools/exp_lzma2_runs.py [STEPS] [--runs N] [--kib N] [--key N] [--label NAME] [--out FILE.txt]"""
import lzma
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
    out_path, runs, kib, key = opt("--out", None), int(opt("--runs", 16)), int(opt("--kib", 256)), int(opt("--key", 65536))
    label = opt("--label", "this build")
    steps = int(argv[0]) if argv else 10
    if not any(os.path.isdir(os.path.join(p, "swcompression_amd")) for p in sys.path if p):
        sys.path.insert(0, ROOT)
    import torch
    import swcompression_amd as swc
    from swcompression_amd import _lib, corpus
    lib = _lib.load()
    assert swc.device_available(), "no usable gfx950 device"

    dict_size = 1 << 20
    db = corpus.lzma2_dict_byte(dict_size)
    filters = [{"id": lzma.FILTER_LZMA2, "preset": 6, "dict_size": dict_size}]
    payload = corpus.p_text(runs * kib << 10, 1200)
    parts = [payload[i:i + (kib << 10)] for i in range(0, len(payload), kib << 10)]
    many = b"".join(lzma.compress(p, format=lzma.FORMAT_RAW, filters=filters)[:-1] for p in parts) + b"\0"
    one = lzma.compress(payload, format=lzma.FORMAT_RAW, filters=filters)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    has_key = lib.swc_set_tuning(b"lzma2_run_bytes", 0) == 0      # (a library from before the key: its rows with the key at 0 only)

    def row(name, stream, k):
        if not has_key and k:
            return None
        if has_key:
            assert lib.swc_set_tuning(b"lzma2_run_bytes", k) == 0
        try:
            assert swc.LZMA2.decompress_raw(stream, db) == (payload, len(stream)), "wrong result"      # warm-up, discarded
            at = [lib.swc_stat(s) for s in (b"launches", b"units", b"lzma2_run_fallbacks")]
            ms = []
            for _ in range(steps):
                t0 = time.perf_counter()
                r = swc.LZMA2.decompress_raw(stream, db)
                ms.append((time.perf_counter() - t0) * 1e3)
                assert r == (payload, len(stream)), "wrong result"
            l, u, f = [max(lib.swc_stat(s) - a, 0) // steps for s, a in zip((b"launches", b"units", b"lzma2_run_fallbacks"), at)]
        finally:
            if has_key:
                lib.swc_set_tuning(b"lzma2_run_bytes", 0)
        mean, sigma = statistics.mean(ms), statistics.pstdev(ms)
        say("%-22s %10.2f +- %-8.2f ms  %8.2f MB/s   %d launches, %d units, %d fallbacks per call"
            % (name, mean, sigma, len(payload) / mean / 1e3, l, u, f))
        return mean

    say("%s: swc_lzma2_decompress, %d x %d KiB of P-text (%d -> %d bytes in %d runs, %d bytes as one run); %s"
        % (label, runs, kib, len(payload), len(many), runs, len(one), torch.cuda.get_device_name(0)))
    say("%d timed calls after one discarded warm-up call each; mean +- sigma of the host clock around the call" % steps)
    say("library: %s%s" % (os.path.relpath(lib._name, ROOT), "" if has_key else ' (refuses "lzma2_run_bytes": the rows with the key at 0 only)'))
    a = row("%d runs, key 0" % runs, many, 0)
    b = row("%d runs, key %d" % (runs, key), many, key)
    row("1 run, key 0", one, 0)
    row("1 run, key %d" % key, one, key)
    if b is not None:
        say("cut into its runs the stream takes %.2f of the time of the one job" % (b / a))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
