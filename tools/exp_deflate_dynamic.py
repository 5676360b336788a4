"""Deflate.compress with dynamic blocks (SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC = 9) against the static codec (8) on the bench's
deflate_compress_64k workload: 100,000 x 64 KiB, 768 P-text + 256 P-mix distinct buffers, seed 2 -- built by bench.make_batch
so that the figures compare with the bench line.  The two codecs are timed alternately in one process: per codec one warm-up
and STEPS timed steps (mean +- sigma as bench.stats computes them), GiB/s of input, the compression ratio, and every stream of
the last step decoded again on the device (bench.verify_compressed_units).

    python tools/exp_deflate_dynamic.py [STEPS] [N_UNITS]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    import torch
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    w8 = bench.WORKLOADS["deflate_compress_64k"]
    n_units = int(sys.argv[2]) if len(sys.argv) > 2 else w8["n_units"]
    ws = {8: w8, 9: dict(w8, codec="deflate_compress_dynamic")}
    batches = {}
    for codec, w in ws.items():
        batches[codec] = bench.make_batch("deflate_compress_64k", w, w8["parts"], 2, "cuda:0", (0, n_units))
    sum_u = {c: int(sum(len(b[2][i]) for i in b[0].unit_index)) for c, b in batches.items()}
    for c, (b, _, _, _) in batches.items():   # one warm-up each
        b.launch()
    torch.cuda.synchronize()
    ms = {8: [], 9: []}
    for k in range(steps):
        for c, (b, _, _, _) in batches.items():
            if k == steps - 1:
                b.wipe_results()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            b.launch()
            e.record()
            torch.cuda.synchronize()
            ms[c].append(s.elapsed_time(e))
    out = {"workload": "deflate_compress_64k", "n_units": n_units, "steps": steps}
    for c, (b, raw, plains, _) in batches.items():
        st = bench.stats(ms[c], 1)
        r = b.results()
        out["codec_%d" % c] = {"step_ms": st["mean_ms"], "sigma_ms": st["sigma_ms"], "min_ms": st["min_ms"], "max_ms": st["max_ms"],
                               "GiBps_input": sum_u[c] / (st["mean_ms"] / 1e3) / 2**30, "out_bytes": int(r["out_len"].sum()),
                               "verify": bench.verify_compressed_units(b, plains, torch, codec="deflate")}
    out["size_9_over_8"] = out["codec_9"]["out_bytes"] / out["codec_8"]["out_bytes"]
    out["time_9_over_8"] = out["codec_9"]["step_ms"] / out["codec_8"]["step_ms"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
