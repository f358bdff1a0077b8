"""bench.py --dump-outputs: the arrays land as float64 .npy files, whole below the size limit and as the same fixed,
seeded sample (with its indices) above it. CPU only: the writer is called directly."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_small_outputs_are_written_whole(tmp_path):
    x = np.linspace(-1.0, 1.0, 1001)
    bench.dump_outputs(str(tmp_path / "d"), {"dx": x})
    y = np.load(tmp_path / "d" / "dx.npy")
    assert y.dtype == np.float64 and np.array_equal(x, y)
    assert not os.path.exists(tmp_path / "d" / "dx_index.npy")


def test_large_outputs_are_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 1000)
    x = np.arange(5000, dtype=np.float64) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"dx": x})
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in ("dx.npy", "dx_index.npy"))  # .npy header: 128 bytes
    assert total <= bench.DUMP_LIMIT_BYTES
    idx = np.load(tmp_path / "a" / "dx_index.npy")
    y = np.load(tmp_path / "a" / "dx.npy")
    assert idx.dtype == np.float64 and y.dtype == np.float64 and idx.size == y.size > 0
    assert np.all(np.diff(idx) > 0) and np.array_equal(y, x[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "dx_index.npy"))
    assert np.array_equal(y, np.load(tmp_path / "b" / "dx.npy"))
