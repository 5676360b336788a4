"""bench.py on the device at a reduced scale: a plain run times exactly --steps steps and dumps what its last step
computed (the same arrays from run to run, every member's CRC-32 and sampled bytes equal to the payload's); --full still
verifies every unit and times the kernels one by one."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 0.02


def _run(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", str(SCALE)] + list(args),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    from swcompression_amd import corpus
    lines = [_run("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / k)) for k in ("a", "b")]
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["metric"] == "decompressed GiB/s" and d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
        assert abs(d["value"] - d["config"]["decompressed_bytes_per_gpu"] / 2**30 / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
        for k in ("cpu_baseline", "per_codec_summary", "units_verified", "config1_latency_ms", "full"):
            assert k not in d, k
        assert "per_kernel_ms" not in d["roofline"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "output_sample.npy" in names and "crc32.npy" in names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10**6
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert a[n[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(a[n[:-4]], np.load(tmp_path / "b" / n)), n
    # what the last step computed is the payload: statuses, lengths, the device CRC-32 of every member, the sampled bytes
    parts = [(c, max(2, int(k * SCALE))) for c, k in (("text", 4096),)]
    _, plains = corpus.build_units_mixed("gzip", parts, 65536, seed=2)
    n = len(a["status"])
    unit = np.arange(n) % len(plains)
    assert n == lines[0]["config"]["units_per_gpu"] and not a["status"].any()
    assert np.array_equal(a["out_len"], np.array([len(plains[u]) for u in unit], dtype=np.float64))
    assert np.array_equal(a["crc32"], np.array([zlib.crc32(plains[u]) for u in unit], dtype=np.float64))
    for row, j in zip(a["output_sample"], a["output_sample_jobs"].astype(np.int64)):
        p = np.frombuffer(plains[unit[j]], dtype=np.uint8)
        assert np.array_equal(row[:len(p)], p) and not row[len(p):].any()


@pytest.mark.gpu
def test_full_run_keeps_the_verification_and_the_kernel_times():
    d = _run("--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "0.5")
    assert d["steps"] == 2 and d["units_verified"] == d["config"]["units_per_gpu"]
    assert set(d["roofline"]["per_kernel_ms"]) >= {"swc_inflate_sync_kernel", "swc_lz_copy_kernel", "swc_crc32_kernel"}
    assert d["cpu_baseline"]["value"] > 0 and d["config1_latency_ms"] > 0 and d["full"]
