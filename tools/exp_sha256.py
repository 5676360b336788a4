"""SHA-256 on the device (swc_batch_sha256: one job per lane, csrc/sha256_lane.h) against one host thread, and sets of .xz archives
through swc_unarchive_many.

    kernel rows    n jobs of 64 KiB and of 1 MiB, n in 1, 16, 32, 64, 256, 1,024, 16,384, at distinct addresses of one buffer of random bytes:
                   device events around swc_batch_sha256 (one discarded call, then STEPS: the least and the mean), and beside it the
                   time ONE host thread takes with swc_sha256 over the same bytes (measured over at most 256 MiB of them and scaled
                   by the byte count: the host function is linear in it) plus the digests' 32 n bytes at 50 GB/s on the way down.
                   The first and the last digest are compared with hashlib.
    archive rows   the 48-archive set of tests/test_gpu_sha256.py and 256 single-block --check=sha256 archives of 64 KiB of text, through
                   swc_unarchive_many("xz"): wall time of a call on the host clock (it ends with the results on the host) and the
                   launches it issues (swc_stat), with "sha256_device_min_units" at 1 (digests from the device), as shipped, and at
                   2^20 (digests on the host).  A library without the key runs one row: to measure an older build put its package first
                   on PYTHONPATH.

    python tools/exp_sha256.py [STEPS] [--label NAME] [--out FILE.json] [--no-kernel]
    python tools/exp_sha256.py --table THIS.json [PARENT.json]        the text of profiles/sha256.txt"""
import ctypes as C
import hashlib
import json
import lzma
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 16, 32, 64, 256, 1024, 16384)
SIZES = (64 << 10, 1 << 20)
HOST_SAMPLE = 256 << 20
SHIPPED = 32   # the library's default of "sha256_device_min_units"


def table(paths):
    cols = [json.load(open(p)) for p in paths]
    this = cols[0]
    lines = []
    if this.get("kernel"):
        lines.append("swc_batch_sha256, %s: kernel time (device events, least / mean of %d) against one host thread (swc_sha256 + 32 n bytes down)"
                     % (this["device"], this["steps"]))
        lines.append("%10s %8s %14s %14s %12s %14s %12s" % ("job bytes", "jobs", "device least ms", "device mean ms", "device GB/s", "host thread ms", "host / device"))
        for r in this["kernel"]:
            lines.append("%10d %8d %14.3f %14.3f %12.3f %14.3f %12.2f" % (r["size"], r["n"], r["dev_min_ms"], r["dev_mean_ms"],
                                                                         r["size"] * r["n"] / r["dev_min_ms"] / 1e6, r["host_ms"], r["host_ms"] / r["dev_min_ms"]))
        lines.append("host thread: %.1f MB/s (swc_sha256 over %d MiB)" % (this["host_mb_s"], this["host_sample"] >> 20))
        for size in SIZES:
            ok = [r["n"] for r in this["kernel"] if r["size"] == size and r["host_ms"] > r["dev_min_ms"]]
            lines.append("jobs of %d bytes: the device is below the host thread from n = %s on" % (size, min(ok) if ok else "(never)"))
        lines.append("")
    lines.append("swc_unarchive_many(\"xz\"): wall ms per call (mean +- sigma of %s), launches per call" % " / ".join(str(c["steps"]) for c in cols))
    for c in cols:
        for r in c["archives"]:
            lines.append("%-28s %-34s %10.2f +- %-7.2f %5d launches, %d digests from the device"
                         % (c["label"], r["shape"], r["mean_ms"], r["sigma_ms"], r["launches"], r["device_units"]))
    return "\n".join(lines)


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--table":
        print(table(argv[1:]))
        return

    def opt(name, default):
        if name in argv:
            v = argv[argv.index(name) + 1]
            del argv[argv.index(name):argv.index(name) + 2]
            return v
        return default
    out_path, label = opt("--out", None), opt("--label", "this build")
    kernel = "--no-kernel" not in argv
    argv = [a for a in argv if a != "--no-kernel"]
    steps = int(argv[0]) if argv else 5
    if not any(os.path.isdir(os.path.join(p, "swcompression_amd")) for p in sys.path if p):
        sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import swcompression_amd as swc
    from swcompression_amd import _lib, corpus
    from swcompression_amd.batch import JOB_DTYPE
    lib = _lib.load()
    dev = torch.device("cuda:0")
    res = {"label": label, "steps": steps, "device": torch.cuda.get_device_name(0), "kernel": [], "archives": []}

    if kernel and hasattr(lib, "swc_batch_sha256"):
        sample = np.random.default_rng(7).integers(0, 256, HOST_SAMPLE, dtype=np.uint8).tobytes()
        dg = C.create_string_buffer(32)
        lib.swc_sha256(sample, 1 << 20, dg)
        t0 = time.perf_counter()
        lib.swc_sha256(sample, len(sample), dg)
        host_s_per_byte = (time.perf_counter() - t0) / len(sample)
        res["host_mb_s"], res["host_sample"] = 1e-6 / host_s_per_byte, HOST_SAMPLE
        for size in SIZES:
            for n in NS:
                total = size * n
                buf = torch.randint(0, 256, (total + 16,), dtype=torch.uint8, device=dev)
                jobs = np.zeros(n, dtype=JOB_DTYPE)
                jobs["out"] = buf.data_ptr() + np.arange(n, dtype=np.uint64) * np.uint64(size)
                jobs["out_cap"] = jobs["out_len"] = size
                d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
                d_dg = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
                opts = _lib.SwcBatchOpts(0, torch.cuda.current_stream(dev).cuda_stream, 0, 0)
                ms = []
                for k in range(steps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    st = lib.swc_batch_sha256(d_jobs.data_ptr(), n, d_dg.data_ptr(), C.byref(opts))
                    e1.record()
                    torch.cuda.synchronize(dev)
                    assert st == 0
                    if k:
                        ms.append(e0.elapsed_time(e1))
                got = d_dg.cpu().numpy()
                for i in (0, n - 1):
                    assert got[32 * i:32 * i + 32].tobytes() == hashlib.sha256(buf[i * size:(i + 1) * size].cpu().numpy().tobytes()).digest()
                host_ms = (total * host_s_per_byte + 32 * n / 50e9) * 1e3
                res["kernel"].append({"size": size, "n": n, "dev_min_ms": min(ms), "dev_mean_ms": statistics.mean(ms), "host_ms": host_ms})
                print("kernel %8d x %6d: %10.3f ms least, host thread %10.3f ms" % (size, n, min(ms), host_ms), flush=True)
                del buf, d_jobs, d_dg

    from test_gpu_sha256 import _archive_set
    sets = [("48 mixed archives", _archive_set()[0]),
            ("256 x 64 KiB single-block", [lzma.compress(corpus.p_text(65536, 3000 + i), check=lzma.CHECK_SHA256, preset=1) for i in range(256)])]
    has_key = lib.swc_set_tuning(b"sha256_device_min_units", SHIPPED) == 0
    for name, archives in sets:
        for key in ((1, SHIPPED, 1 << 20) if has_key else (None,)):
            if key is not None:
                assert lib.swc_set_tuning(b"sha256_device_min_units", key) == 0
            first = swc.unarchive_many("xz", archives)
            ts = []
            l0, u0 = lib.swc_stat(b"launches"), max(lib.swc_stat(b"sha256_device_units"), 0)
            for _ in range(steps):
                t0 = time.perf_counter()
                got = swc.unarchive_many("xz", archives)
                ts.append((time.perf_counter() - t0) * 1e3)
                assert got == first
            shape = name + ("" if key is None else ", min_units %d" % key)
            res["archives"].append({"shape": shape, "mean_ms": statistics.mean(ts), "sigma_ms": statistics.pstdev(ts),
                                    "launches": (lib.swc_stat(b"launches") - l0) // steps,
                                    "device_units": (max(lib.swc_stat(b"sha256_device_units"), 0) - u0) // steps})
            print("%-44s %10.2f ms, %d launches" % (shape, res["archives"][-1]["mean_ms"], res["archives"][-1]["launches"]), flush=True)
    if has_key:
        lib.swc_set_tuning(b"sha256_device_min_units", SHIPPED)
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
