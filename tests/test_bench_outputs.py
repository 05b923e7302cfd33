"""bench.py --dump-outputs on the CPU: the placement records of a step become one float64 .npy per field, the same
files for the same records, and a step too large for 64 MB is cut to a fixed sample of its pods."""
import os

import numpy as np

import bench
from koordinator_amd import abi


def _records(n, seed=3):
    rng = np.random.default_rng(seed)
    out = np.zeros(n, abi.PLACEMENT_DTYPE)
    out["node"] = rng.integers(-1, 50_000, n)
    out["feasible"] = rng.integers(0, 50_000, n)
    out["score"] = rng.integers(0, 300, n)
    out["ties"] = rng.integers(0, 200, n)
    out["flags"] = rng.integers(0, 1 << 12, n)
    return out


def test_dump_outputs_one_float64_array_per_field(tmp_path):
    out = _records(257)
    d = str(tmp_path / "a")
    written = bench.dump_outputs(d, out)
    assert sorted(written) == ["feasible", "flags", "node", "score", "ties"]
    for f in written:
        a = np.load(os.path.join(d, f + ".npy"))
        assert a.dtype == np.float64 and a.shape == (257,)
        assert np.array_equal(a, out[f].astype(np.float64))
        assert np.array_equal(a.astype(out.dtype[f]), out[f])   # exact: nothing rounded
    assert np.array_equal(np.load(os.path.join(d, "rows.npy")), np.arange(257))
    # the same records again: the same files
    d2 = str(tmp_path / "b")
    bench.dump_outputs(d2, out.copy())
    for name in os.listdir(d):
        assert np.array_equal(np.load(os.path.join(d, name)), np.load(os.path.join(d2, name)))


def test_dump_outputs_with_extension_records(tmp_path):
    out = _records(16)
    ext = np.zeros(16, abi.EXT_PLACEMENT_DTYPE)
    ext["gpu_count"] = np.arange(16)
    d = str(tmp_path / "c5")
    written = bench.dump_outputs(d, out, ext)
    assert "ext_gpu_count" in written and "ext_pad0" not in written
    assert np.array_equal(np.load(os.path.join(d, "ext_gpu_count.npy")), np.arange(16, dtype=np.float64))
    assert np.load(os.path.join(d, "ext_gpu_per_instance.npy")).shape == (16, abi.GS_NUM_GPU_RES)


def test_dump_outputs_samples_a_step_past_64_mb(tmp_path, monkeypatch):
    out = _records(4096)
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 48 * 1000)   # 48 B per record and row index: 1000 rows
    d = str(tmp_path / "s")
    bench.dump_outputs(d, out)
    rows = np.load(os.path.join(d, "rows.npy")).astype(np.int64)
    assert len(rows) == 1000 and np.all(np.diff(rows) > 0) and rows[-1] < 4096
    assert np.array_equal(np.load(os.path.join(d, "node.npy")), out["node"][rows].astype(np.float64))
    bench.dump_outputs(str(tmp_path / "s2"), out)
    assert np.array_equal(np.load(os.path.join(str(tmp_path / "s2"), "rows.npy")), rows)
    total = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
    assert total <= 48 * 1000 + 6 * 128   # the arrays plus the .npy headers
