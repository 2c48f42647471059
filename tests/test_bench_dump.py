"""bench.py --dump-outputs on the host: the files it writes for a frame, whole or sampled (no GPU needed)."""
import os

import numpy as np

import bench


def _frame(W, H, seed):
    rng = np.random.default_rng(seed)
    s = rng.random((W * H, 3), dtype=np.float32)
    return s, s * s, rng.integers(0, 300, W * H).astype(np.int32)


def test_small_frame_is_written_whole(tmp_path):
    W, H = 40, 24
    s, s2, c = _frame(W, H, 1)
    names = bench.dump_outputs(str(tmp_path), s, s2, c, W, H)
    assert names == ["radiance_sum", "radiance_sum2", "sample_count"]
    a, a2, ac = (np.load(tmp_path / f"{n}.npy") for n in names)
    assert a.dtype == a2.dtype == ac.dtype == np.float32
    assert np.array_equal(a, s.reshape(H, W, 3)) and np.array_equal(a2, s2.reshape(H, W, 3))
    assert np.array_equal(ac, c.reshape(H, W).astype(np.float32))


def test_large_frame_is_a_fixed_sample_within_the_cap(tmp_path, monkeypatch):
    W, H = 64, 50
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 36 * 1000)        # room for 1000 of the 3200 pixels
    s, s2, c = _frame(W, H, 2)
    d1, d2 = tmp_path / "a", tmp_path / "b"
    assert bench.dump_outputs(str(d1), s, s2, c, W, H) == ["pixel_index", "radiance_sum", "radiance_sum2", "sample_count"]
    bench.dump_outputs(str(d2), s, s2, c, W, H)
    assert sum(os.path.getsize(d1 / f) - 128 for f in os.listdir(d1)) <= 36 * 1000     # (128 B: each file's .npy header)
    idx = np.load(d1 / "pixel_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 1000 and (np.diff(idx) > 0).all()
    i = idx.astype(np.int64)
    assert np.array_equal(np.load(d1 / "radiance_sum.npy"), s[i]) and np.array_equal(np.load(d1 / "radiance_sum2.npy"), s2[i])
    assert np.array_equal(np.load(d1 / "sample_count.npy"), c[i].astype(np.float32))
    for f in os.listdir(d1):                                        # the same sample every time
        assert np.array_equal(np.load(d1 / f), np.load(d2 / f))
