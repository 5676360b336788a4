"""LZ4 frames with dependent (linked) blocks through the single-shot entry points: what a call costs, end to end on the host clock
(every call ends with a device synchronise and the copy of the result).  liblz4 frames of P-text (corpus.lz4f_frame, linked):

    decompress 16 x 64 KiB     LZ4.decompress on one frame of 16 blocks of 64 KiB
    decompress 64 x 64 KiB     ... of 64 blocks of 64 KiB
    decompress 4 x 4 MiB       ... of 4 blocks of 4 MiB
    unarchive_many 1024        swc_unarchive_many on 1,024 frames of 16 x 64 KiB (8 distinct payloads)

Per shape one discarded warm-up call and STEPS timed calls: mean and sigma in ms, the launches one call issues (swc_stat), and
the result compared with the payload.  The tool uses nothing that an older library lacks, so the same file measures an older
build of the library: put that build's package first on PYTHONPATH.

    python tools/exp_lz4_linked.py [STEPS] [--frames N] [--label NAME] [--out FILE.json]
    python tools/exp_lz4_linked.py --table PARENT.json THIS.json      the two columns side by side, as in profiles/lz4_linked.txt"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(parent, this):
    a, b = json.load(open(parent)), json.load(open(this))
    lines = ["%-28s %26s %26s %8s" % ("shape (ms per call)", a["label"], b["label"], "factor")]
    for ra, rb in zip(a["rows"], b["rows"]):
        assert ra["shape"] == rb["shape"]
        cell = lambda r: "%10.2f +- %-7.2f (%d launches)" % (r["mean_ms"], r["sigma_ms"], r["launches"])   # noqa: E731
        lines.append("%-28s %26s %26s %7.1fx" % (ra["shape"], cell(ra), cell(rb), ra["mean_ms"] / rb["mean_ms"]))
    lines.append("steps: %d / %d after one discarded warm-up call each; mean +- sigma of the host clock around the call" % (a["steps"], b["steps"]))
    lines.append("device: %s" % b["device"])
    return "\n".join(lines)


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--table":
        print(table(argv[1], argv[2]))
        return

    def opt(name, default):
        if name in argv:
            v = argv[argv.index(name) + 1]
            del argv[argv.index(name):argv.index(name) + 2]
            return v
        return default
    out_path, label, n_frames = opt("--out", None), opt("--label", "this build"), int(opt("--frames", 1024))
    steps = int(argv[0]) if argv else 10
    if not any(os.path.isdir(os.path.join(p, "swcompression_amd")) for p in sys.path if p):
        sys.path.insert(0, ROOT)
    import torch
    import swcompression_amd as swc
    from swcompression_amd import _lib, corpus
    lib = _lib.load()
    assert swc.device_available(), "no usable gfx950 device"

    def timed(fn, check):
        assert check(fn()), "wrong result"      # warm-up, discarded
        l0 = lib.swc_stat(b"launches")
        ms = []
        for _ in range(steps):
            t0 = time.perf_counter()
            r = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
            assert check(r), "wrong result"
        return statistics.mean(ms), statistics.pstdev(ms), (lib.swc_stat(b"launches") - l0) // steps

    rows = []
    for name, code, size in (("decompress 16 x 64 KiB", 4, 16 << 16), ("decompress 64 x 64 KiB", 4, 64 << 16), ("decompress 4 x 4 MiB", 7, 4 << 22)):
        payload = corpus.p_text(size, 700 + code)
        frame = corpus.lz4f_frame(payload, code, True, True)
        mean, sigma, launches = timed(lambda: swc.LZ4.decompress(frame), lambda r: r == payload)
        rows.append({"shape": name, "mean_ms": mean, "sigma_ms": sigma, "launches": int(launches), "bytes": size})
        print("%-28s %10.2f +- %.2f ms   %d launches" % (name, mean, sigma, launches), flush=True)
    payloads = [corpus.p_text(16 << 16, 720 + i) for i in range(8)]
    frames = [corpus.lz4f_frame(p, 4, True, True) for p in payloads]
    many = [frames[i % 8] for i in range(n_frames)]
    ok = lambda r: all(st == 0 and out == payloads[i % 8] for i, (st, out) in enumerate(r))   # noqa: E731
    mean, sigma, launches = timed(lambda: swc.unarchive_many("lz4", many), ok)
    name = "unarchive_many %d" % n_frames
    rows.append({"shape": name, "mean_ms": mean, "sigma_ms": sigma, "launches": int(launches), "bytes": n_frames * (16 << 16)})
    print("%-28s %10.2f +- %.2f ms   %d launches" % (name, mean, sigma, launches), flush=True)
    res = {"label": label, "steps": steps, "device": torch.cuda.get_device_name(0), "rows": rows}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
