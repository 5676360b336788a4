"""Deflate streams cut at their flush points: what a decode costs, end to end on the host clock (every call ends with a device
synchronise and the copy of the result).

    own archive, host          GzipArchive.unarchive(GzipArchive.archive(MIB MiB of P-text)): 256 KiB segments joined by empty stored blocks
    own archive, device jobs   the same stream staged in HBM once, one launch of its units (DeviceBatch; the head owns the output)
    sync-flushed, host         a zlib Z_SYNC_FLUSH member of MIB / 8 MiB, flushed every 128 KiB: units that refer to each other, so
                               the run is refused and the stream decoded whole -- what the fallback costs
    sync MIB MiB, ...          a Z_SYNC_FLUSH-every-128-KiB gzip member of MIB MiB -- what default pigz writes -- decoded three ways: with
                               the knob off (one job), as units that stand alone (refused: the joined fallback), and as units that share
                               history ("deflate_units_linked" = 1: one launch, the copy a chain on one wave); a library without the
                               key runs the third row as the second

Per shape one discarded warm-up call and STEPS timed calls: mean and sigma in ms, the launches and fallbacks one call issues
(swc_stat), the result compared with the payload.  The units of the device-resident row are found HERE (the marker rule restated),
and a library without the unit contract -- swc_set_tuning refuses "deflate_unit_bytes" -- runs that row as the single job it would
be there, so the same file measures an older build of the library: put that build's package first on PYTHONPATH.

    python tools/exp_deflate_units.py [STEPS] [--mib N] [--unit-bytes N] [--label NAME] [--out FILE.json]
    python tools/exp_deflate_units.py --table PARENT.json THIS.json [MORE.json ...]     the columns side by side, as in profiles/deflate_units.txt"""
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = b"\x00\x00\xff\xff"


def units_of(raw, unit_bytes):
    """[(offset, length, aux)]: a cut behind every marker that closes a unit of at least unit_bytes, none at the very end."""
    cuts, start, i = [], 0, 0
    while unit_bytes:
        i = raw.find(MARK, i)
        if i < 0:
            break
        if i + 4 < len(raw) and i + 4 - start >= unit_bytes:
            cuts.append(i + 4)
            start = i + 4
        i += 1
    edges = [0] + cuts + [len(raw)]
    n = len(edges) - 1
    return [(edges[k], edges[k + 1] - edges[k], (1 if k else 0) | (2 if k + 1 < n else 0)) for k in range(n)]


def table(paths):
    cols = [json.load(open(p)) for p in paths]
    lines = ["%-26s" % "shape (ms per call)" + "".join(" %34s" % c["label"] for c in cols)]
    for i, row in enumerate(cols[0]["rows"]):
        cells = []
        for c in cols:
            r = c["rows"][i]
            assert r["shape"] == row["shape"]
            cells.append(" %12.2f +- %-6.2f (%d l, %d fb)" % (r["mean_ms"], r["sigma_ms"], r["launches"], r["fallbacks"]))
        lines.append("%-26s" % row["shape"] + "".join("%35s" % x for x in cells))
    lines.append("steps: %s after one discarded warm-up call each; mean +- sigma of the host clock around the call; l = launches, fb = fallbacks per call"
                 % " / ".join(str(c["steps"]) for c in cols))
    lines.append("payload: %d MiB of P-text; device: %s" % (cols[-1]["mib"], cols[-1]["device"]))
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
    out_path, label, mib, unit_bytes = opt("--out", None), opt("--label", "this build"), int(opt("--mib", 256)), int(opt("--unit-bytes", 32768))
    steps = int(argv[0]) if argv else 10
    if not any(os.path.isdir(os.path.join(p, "swcompression_amd")) for p in sys.path if p):
        sys.path.insert(0, ROOT)
    import torch
    import swcompression_amd as swc
    from swcompression_amd import _lib, corpus
    from swcompression_amd.batch import DeviceBatch
    lib = _lib.load()
    assert swc.device_available(), "no usable gfx950 device"
    has_units = lib.swc_set_tuning(b"deflate_unit_bytes", unit_bytes) == 0

    def stat(key):
        v = lib.swc_stat(key)
        return max(v, 0)

    def timed(fn, check):
        assert check(fn()), "wrong result"      # warm-up, discarded
        l0, f0 = stat(b"launches"), stat(b"deflate_unit_fallbacks")
        ms = []
        for _ in range(steps):
            t0 = time.perf_counter()
            r = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
            assert check(r), "wrong result"
        return statistics.mean(ms), statistics.pstdev(ms), (stat(b"launches") - l0) // steps, (stat(b"deflate_unit_fallbacks") - f0) // steps

    rows = []

    def row(name, fn, check, size):
        mean, sigma, launches, fallbacks = timed(fn, check)
        rows.append({"shape": name, "mean_ms": mean, "sigma_ms": sigma, "launches": int(launches), "fallbacks": int(fallbacks), "bytes": size})
        print("%-26s %10.2f +- %.2f ms   %d launches, %d fallbacks" % (name, mean, sigma, launches, fallbacks), flush=True)

    payload = corpus.p_text(mib << 20, 800)
    z = swc.GzipArchive.archive(payload)
    row("own archive, host", lambda: swc.GzipArchive.unarchive(z), lambda r: r == payload, len(payload))

    raw = z[10:-8]
    units = units_of(raw, unit_bytes if has_units else 0)
    caps = [max(65536, 6 * n + 1024) for _, n, _ in units] if len(units) > 1 else [len(payload)]
    b = DeviceBatch("deflate", [raw[o:o + n] for o, n, _ in units], caps, aux=[a for _, _, a in units], replicate_inputs=False)
    crc = zlib.crc32(payload)

    def device_jobs():
        b.launch(sync=True)
        return b.results()

    def device_ok(r):
        if not (r["status"] == 0).all() or int(r["out_len"].sum()) != len(payload):
            return False
        first = int(r["out"][0]) - b.d_out.data_ptr()
        return zlib.crc32(b.d_out[first:first + len(payload)].cpu().numpy().tobytes()) == crc
    row("own archive, device jobs", device_jobs, device_ok, len(payload))
    del b

    small = payload[:max(mib // 8, 1) << 20]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    sync = b"".join(c.compress(small[i:i + (128 << 10)]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(small), 128 << 10)) + c.flush()
    member = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + sync + struct.pack("<II", zlib.crc32(small), len(small) & 0xFFFFFFFF)
    row("sync-flushed, host", lambda: swc.GzipArchive.unarchive(member), lambda r: r == small, len(small))

    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    sync = b"".join(c.compress(payload[i:i + (128 << 10)]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(payload), 128 << 10)) + c.flush()
    member = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + sync + struct.pack("<II", crc, len(payload) & 0xFFFFFFFF)
    del sync
    for name, ub, linked in (("sync %d MiB, knob off" % mib, 0, 0), ("sync %d MiB, units joined" % mib, unit_bytes, 0), ("sync %d MiB, units linked" % mib, unit_bytes, 1)):
        if has_units:
            lib.swc_set_tuning(b"deflate_unit_bytes", ub)
        lib.swc_set_tuning(b"deflate_units_linked", linked)      # (refused by a library without the key)
        row(name, lambda: swc.GzipArchive.unarchive(member), lambda r: r == payload, len(payload))
    lib.swc_set_tuning(b"deflate_units_linked", 0)

    res = {"label": label, "steps": steps, "mib": mib, "unit_bytes": unit_bytes if has_units else 0, "device": torch.cuda.get_device_name(0), "rows": rows}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
