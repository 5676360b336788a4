"""The BGZF writer (swc_batch_bgzf_archive, device-resident) on the bench's deflate_compress_64k corpus CONCATENATED: 100,000 x
64 KiB (768 P-text + 256 P-mix distinct buffers, seed 2, the list bench.make_batch tiles), cut at the default block size of 65,280
bytes, with static and with dynamic blocks.  Per form: one warm-up and STEPS timed calls (the whole call between two events, and
the three phases of swc_last_phase_ms: compress | CRC-32 of the chunks | offsets + pack), the file size, and members from the
front and the end of the file decoded again by GzipArchive.multi_unarchive.  Beside them, in the same process, the plain compress
launches of the same buffers (codec 8 and 9 through bench.make_batch: what the bench's ENCODE lines time), so that
"what CRC + offsets + pack add" is a ratio of figures from one run on one box.

    python tools/exp_bgzf.py [STEPS] [N_UNITS] [--no-baseline] [--out FILE]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def timed(torch, fn, steps):
    fn()   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = fn()
        e.record()
        torch.cuda.synchronize()
        ms.append((s.elapsed_time(e), r))
    return ms


def main():
    import torch
    import swcompression_amd as swc
    from swcompression_amd import _lib, batch, corpus
    argv = sys.argv[1:]
    out_path = None
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    args = [a for a in argv if not a.startswith("--")]
    steps = int(args[0]) if args else 5
    w = bench.WORKLOADS["deflate_compress_64k"]
    n_units = int(args[1]) if len(args) > 1 else w["n_units"]
    lib = _lib.load()
    dev = torch.device("cuda:0")
    _, plains = corpus.build_units_mixed("gzip", w["parts"], w["unit"], seed=2)
    nd, unit = len(plains), w["unit"]
    tile = torch.from_numpy(np.frombuffer(b"".join(plains), dtype=np.uint8).copy()).to(dev)
    n_bytes = n_units * unit
    src = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    for o in range(0, n_bytes, nd * unit):
        m = min(nd * unit, n_bytes - o)
        src[o:o + m].copy_(tile[:m])
    bs = 65280
    members = -(-n_bytes // bs)
    dst = torch.empty(lib.swc_bgzf_bound(n_bytes, bs), dtype=torch.uint8, device=dev)
    ws = torch.empty(batch.bgzf_workspace_bytes(n_bytes, bs), dtype=torch.uint8, device=dev)
    res = {"corpus": "deflate_compress_64k concatenated", "n_units": n_units, "input_bytes": n_bytes, "block_size": bs, "members": members,
           "steps": steps, "device": torch.cuda.get_device_name(0)}
    tile_bytes = b"".join(plains)

    def expect(lo, n):   # bytes [lo, lo + n) of the concatenated corpus
        o = lo % len(tile_bytes)
        return (tile_bytes[o:] + tile_bytes * (n // len(tile_bytes) + 1))[:n]
    lib.swc_set_tuning(b"phase_timing", 1)
    try:
        for dynamic in (False, True):
            phases = []

            def call():
                st, total, sizes = batch.bgzf_archive(src, dst, block_size=bs, dynamic=dynamic, workspace=ws)
                assert st == 0, st
                buf = (C.c_float * 8)()
                assert lib.swc_last_phase_ms(buf, 8) == 3
                phases.append([buf[0], buf[1], buf[2]])
                return total, sizes
            ms = timed(torch, call, steps)
            total, sizes = ms[-1][1]
            assert int(sizes.sum()) == total and len(sizes) == members + 1
            # members from the front and from the end, decoded again and compared
            k = min(members, 1100)
            front = int(sizes[:k].sum())
            got = b"".join(swc.GzipArchive.multi_unarchive(dst[:front].cpu().numpy().tobytes()))
            ok = got == expect(0, min(k * bs, n_bytes))
            back = int(sizes[members - k:].sum())
            got = b"".join(swc.GzipArchive.multi_unarchive(dst[total - back:total].cpu().numpy().tobytes()))
            lo = (members - k) * bs
            ok = ok and got == expect(lo, n_bytes - lo)
            ph = np.array(phases[1:])
            call_ms = np.array([m for m, _ in ms])
            res["bgzf_dynamic" if dynamic else "bgzf_static"] = {
                "call_ms": float(call_ms.mean()), "call_sigma_ms": float(call_ms.std()),
                "compress_ms": float(ph[:, 0].mean()), "crc_ms": float(ph[:, 1].mean()), "scan_pack_ms": float(ph[:, 2].mean()),
                "added_over_compress": float((ph[:, 1] + ph[:, 2]).mean() / ph[:, 0].mean()),
                "file_bytes": total, "ratio": n_bytes / total, "GiBps_input": n_bytes / (call_ms.mean() / 1e3) / 2**30,
                "scan_pack_GBps": 2 * total / (ph[:, 2].mean() / 1e3) / 1e9,   # the pack reads the streams once and writes them once
                "verified_members": 2 * k, "verify_ok": bool(ok)}
    finally:
        lib.swc_set_tuning(b"phase_timing", 0)
    del dst, ws, src
    torch.cuda.empty_cache()
    if "--no-baseline" not in sys.argv:   # the plain compress launches of the same buffers, as bench.py --full times them
        for codec, key in (("deflate_compress", "codec_8"), ("deflate_compress_dynamic", "codec_9")):
            b = bench.make_batch("deflate_compress_64k", dict(w, codec=codec), w["parts"], 2, "cuda:0", (0, n_units))[0]
            ms = np.array([m for m, _ in timed(torch, b.launch, steps)])
            res[key] = {"step_ms": float(ms.mean()), "sigma_ms": float(ms.std())}
            del b
            torch.cuda.empty_cache()
        res["bgzf_static_over_codec_8"] = res["bgzf_static"]["call_ms"] / res["codec_8"]["step_ms"]
        res["bgzf_dynamic_over_codec_9"] = res["bgzf_dynamic"]["call_ms"] / res["codec_9"]["step_ms"]
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
