"""LZMA2.compress on the device (SWC_CODEC_LZMA2_COMPRESS = 10) on the mix of the bench's deflate_compress_64k workload: N x 64 KiB,
768 P-text + 256 P-mix distinct buffers, seed 2 (corpus.build_units_mixed, as bench.make_batch builds them), every job at its own
device address.  One warm-up and STEPS timed steps (mean +- sigma as bench.stats computes them), GiB/s of input, the compression
ratio, every run of the last step decoded again on the device by the engine's own LZMA2 decoder (sizes and CRC-32), the size
against the dynamic Deflate codec (9) on the same buffers and against liblzma's preset 0 with the same dictionary of 64 KiB.

    python tools/exp_lzma2_compress.py [N_UNITS] [STEPS]

Variants of the kernel (lc, hash bits) are builds of their own: SWC_EXTRA_HIPCC_FLAGS="-DSWC_LZMAC_LC=0" or
"-DSWC_LZMAC_HASH_BITS=13" python -m swcompression_amd.build --force, then this tool."""
import json
import lzma
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    import numpy as np
    import torch
    from swcompression_amd import corpus
    from swcompression_amd.batch import DeviceBatch
    n_units = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    w = bench.WORKLOADS["deflate_compress_64k"]
    _, plains = corpus.build_units_mixed("gzip", w["parts"], w["unit"], seed=2)
    nd = len(plains)
    tile = -(-n_units // nd)
    caps = [len(p) + 3 * -(-len(p) // 65536) + 1 for p in plains]
    b = DeviceBatch("lzma2_compress", plains, caps, tile=tile, select=(0, n_units))
    total_in = int(sum(len(plains[i]) for i in b.unit_index))
    b.launch(sync=True)   # warm-up
    ms = []
    for k in range(steps):
        if k == steps - 1:
            b.wipe_results()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        b.launch()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    st = bench.stats(ms, 1)
    r = b.results()
    assert (r["status"] == 0).all(), sorted(set(r["status"].tolist()))
    out_bytes = int(r["out_len"].sum())
    # every run decoded again where it lies
    dec = DeviceBatch("lzma2", [b"\x00"] * nd, [len(p) for p in plains], aux=[8] * nd, tile=tile, select=(0, n_units))
    jobs = dec._jobs_host.copy()
    jobs["in"] = r["out"]
    jobs["in_len"] = r["out_len"]
    dec._jobs_host = jobs
    dec.d_jobs.copy_(torch.from_numpy(jobs.view(np.uint8)).to(dec.device))
    dec.launch(sync=True)
    d = dec.results()
    want_len = np.array([len(p) for p in plains], dtype=np.uint64)[dec.unit_index]
    want_crc = np.array([zlib.crc32(p) & 0xFFFFFFFF for p in plains], dtype=np.uint32)[dec.unit_index]
    ok = bool((d["status"] == 0).all()) and bool((d["out_len"] == want_len).all()) and bool((dec.crc32() == want_crc).all())
    if not ok:
        raise SystemExit("round trip of the compressed runs failed")
    # sizes on the distinct buffers: this codec, the dynamic Deflate codec, liblzma's preset 0
    k = min(nd, n_units)
    ours = int(r["out_len"][:k].sum())
    d9 = DeviceBatch("deflate_compress_dynamic", plains[:k], [len(p) + len(p) // 8 + 32 for p in plains[:k]])
    d9.launch(sync=True)
    r9 = d9.results()
    assert (r9["status"] == 0).all()
    flt = [{"id": lzma.FILTER_LZMA2, "preset": 0, "dict_size": 65536}]
    xz0 = sum(len(lzma.compress(p, format=lzma.FORMAT_RAW, filters=flt)) for p in plains[:k])
    print(json.dumps({"workload": "N x 64 KiB of the deflate_compress_64k mix", "n_units": n_units, "steps": steps,
                      "step_ms": st["mean_ms"], "sigma_ms": st["sigma_ms"], "min_ms": st["min_ms"], "max_ms": st["max_ms"],
                      "GiBps_input": total_in / (st["mean_ms"] / 1e3) / 2**30, "out_bytes": out_bytes, "ratio": total_in / out_bytes,
                      "verify": "%d runs decoded on the device: sizes and CRC-32 == the payloads'" % n_units,
                      "distinct_units_compared": k, "bytes_lzma2": ours, "bytes_deflate_dynamic": int(r9["out_len"].sum()),
                      "size_over_deflate_dynamic": ours / int(r9["out_len"].sum()), "bytes_liblzma_preset0": xz0,
                      "size_over_liblzma_preset0": ours / xz0}, indent=1))


if __name__ == "__main__":
    main()
