"""CPU: bench.py --dump-outputs stays under its size limit with a fixed, seeded sample of every array's rows."""
import os

import numpy as np

import bench


def test_dump_outputs_small_arrays_are_written_whole(tmp_path):
    x = np.arange(10, dtype=np.float32)
    q = np.arange(30, dtype=np.float32).reshape(10, 3)
    bench.dump_outputs(str(tmp_path), {"x": x, "q": q})
    assert np.array_equal(np.load(str(tmp_path / "x.npy")), x)
    assert np.array_equal(np.load(str(tmp_path / "q.npy")), q)


def test_dump_outputs_large_arrays_are_sampled_the_same_way(tmp_path):
    n = 5_000_000  # x + q = 80 MB of float32 (every value an exact integer)
    arrays = {"x": np.arange(n, dtype=np.float32), "q": np.arange(3 * n, dtype=np.float32).reshape(n, 3)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    files = [tmp_path / s / (k + ".npy") for s in "ab" for k in arrays]
    assert sum(os.path.getsize(str(f)) for f in files[:2]) <= 64_000_000
    for k in arrays:
        a, b = np.load(str(tmp_path / "a" / (k + ".npy"))), np.load(str(tmp_path / "b" / (k + ".npy")))
        assert a.dtype == np.float32 and 0 < len(a) < n and np.array_equal(a, b), k
    # every array keeps the same rows, in order
    rows = np.load(str(tmp_path / "a" / "x.npy")).astype(np.int64)
    assert np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(str(tmp_path / "a" / "q.npy"))[:, 0].astype(np.int64), 3 * rows)
