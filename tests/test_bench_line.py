"""bench.py prints ONE compact headline object as the LAST line of stdout (round 5's full object had grown to 24.7 KB on
one line and the driver's record came back `parsed: null`).  This runs the formatter on a canned full result -- round 5's
own (profiles/r05z_bench_full.json) -- and checks size, validity and the keys the driver's record held in rounds 1-4."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_compact_line_is_small_valid_and_complete():
    full = json.load(open(os.path.join(ROOT, "profiles", "r05z_bench_full.json")))
    assert len(json.dumps(full)) > 20000          # (the canned object is the one that broke the record)
    full["full"] = "bench_full.json"
    line = _bench().compact_line(full)
    assert "\n" not in line and len(line) < 4096, len(line)
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert k in d, k
    assert d["vs_baseline"] is None and d["dtype"] == "u8" and d["higher_is_better"] is True
    for k in ("workload", "codec", "units_per_gpu", "unit_bytes", "compressed_bytes_per_gpu", "decompressed_bytes_per_gpu"):
        assert k in d["config"], k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "kernel", "kernel_ms", "algorithmic_bytes_per_launch",
              "per_kernel_ms", "dominant_kernel", "dominant_kernel_frac"):
        assert k in d["roofline"], k
    assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-4
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert set(d["per_codec_summary"]) == set(full["per_codec"])
    for name, (ms, gibs, frac) in d["per_codec_summary"].items():
        assert abs(ms - full["per_codec"][name]["ms_per_step"]) < 0.01 and 0 < frac < 1
    # the headline figures are the full object's
    assert abs(d["value"] - full["value"]) < 1e-3 and abs(d["ms_per_step"] - full["ms_per_step"]) < 1e-3


def test_compact_line_without_the_optional_parts():
    """N > 1 ranks / --no-cpu-baseline / --no-per-codec runs carry no cpu_baseline, per_codec or latency line."""
    full = json.load(open(os.path.join(ROOT, "profiles", "r05z_bench_full.json")))
    for k in ("cpu_baseline", "cpu_baseline_all_cores", "cpu_context", "per_codec", "config1_latency", "archive_paths", "lz4_streamed"):
        full.pop(k, None)
    full["roofline"].pop("per_kernel_ms")
    d = json.loads(_bench().compact_line(full))
    assert "cpu_baseline" not in d and "per_codec_summary" not in d and d["roofline"]["frac"] > 0


class _HostBatch:
    """The parts of a DeviceBatch that bench.dump_outputs reads, on host tensors: `n` jobs with `cap` bytes of output each."""

    def __init__(self, n, cap, seed=7):
        import numpy as np
        import torch
        from swcompression_amd.batch import JOB_DTYPE
        rng = np.random.Generator(np.random.PCG64(seed))
        self.n = n
        self.caps = np.full(n, cap, dtype=np.uint64)
        self._out_off = np.arange(n, dtype=np.int64) * cap
        self.d_out = torch.from_numpy(rng.integers(0, 256, size=n * cap + 16, dtype=np.uint8))
        self.jobs = np.zeros(n, dtype=JOB_DTYPE)
        self.jobs["out_cap"] = cap
        self.jobs["out_len"] = rng.integers(0, cap + 1, size=n)
        self.jobs["in_consumed"] = rng.integers(1, 1 << 40, size=n)
        self.jobs["status"] = rng.integers(0, 3, size=n)
        self._crc_buf = torch.from_numpy(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.int32))

    def results(self):
        return self.jobs.copy()


def test_dump_outputs_writes_the_last_step_as_float_arrays(tmp_path):
    import numpy as np
    m = _bench()
    b = _HostBatch(40, 256)
    m.dump_outputs(str(tmp_path / "a"), b, gzip_crc=True)
    m.dump_outputs(str(tmp_path / "b"), b, gzip_crc=True)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(n + ".npy" for n in ("status", "out_len", "in_consumed", "crc32", "output_sample", "output_sample_jobs"))
    d = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n, a in d.items():
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, np.load(tmp_path / "b" / (n + ".npy"))), n     # the same sample from run to run
    assert np.array_equal(d["status"], b.jobs["status"]) and np.array_equal(d["out_len"], b.jobs["out_len"].astype(np.float64))
    assert np.array_equal(d["in_consumed"], b.jobs["in_consumed"].astype(np.float64))
    assert np.array_equal(d["crc32"], b._crc_buf.numpy().view(np.uint32).astype(np.float64))   # exact: every uint32 is a float64
    jobs = d["output_sample_jobs"].astype(np.int64)
    assert len(jobs) == 40 and np.array_equal(jobs, np.arange(40))      # small enough: every job
    out = b.d_out.numpy()
    for row, i in zip(d["output_sample"], jobs):
        n = int(b.jobs["out_len"][i])
        assert np.array_equal(row[:n], out[i * 256:i * 256 + n]) and not row[n:].any()
    m.dump_outputs(str(tmp_path / "c"), b, gzip_crc=False)
    assert not (tmp_path / "c" / "crc32.npy").exists()


def test_dump_outputs_stays_within_its_size_limit(tmp_path, monkeypatch):
    import numpy as np
    m = _bench()
    monkeypatch.setattr(m, "DUMP_LIMIT", 20000)
    b = _HostBatch(300, 1024)
    m.dump_outputs(str(tmp_path), b, gzip_crc=True)
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= 20000 + 6 * 128    # (+ the .npy headers)
    jobs = np.load(tmp_path / "output_sample_jobs.npy").astype(np.int64)
    assert 1 <= len(jobs) < 300 and np.all(np.diff(jobs) > 0) and jobs.max() < 300
    assert _bench().DUMP_LIMIT + 6 * 128 <= 64 * 10**6      # the real limit: 64 MB in all, headers included


def test_steps_full_and_dump_options(monkeypatch):
    import sys
    m = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = m.parse_args()
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--full", "--dump-outputs", "out"])
    a = m.parse_args()
    assert a.full is True and a.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    import pytest
    with pytest.raises(SystemExit):
        m.parse_args()
