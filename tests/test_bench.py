"""bench.py --dump-outputs on the host: the image as written, a large image as a fixed sample within the 64 MB budget."""
import os

import numpy as np

import bench


def test_dump_outputs_writes_the_whole_image_when_it_fits(tmp_path):
    img = np.random.default_rng(1).random((1080, 1920, 3), dtype=np.float32)
    bench.dump_outputs(str(tmp_path), img)
    assert sorted(os.listdir(tmp_path)) == ["image.npy"]
    got = np.load(tmp_path / "image.npy")
    assert got.dtype == np.float32 and got.shape == img.shape and np.array_equal(got, img)


def test_dump_outputs_samples_a_large_image_the_same_pixels_every_run(tmp_path):
    img = np.random.default_rng(2).random((2160, 3840, 3), dtype=np.float32)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), img)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["image_sample.npy", "image_sample_pixels.npy"]
    assert sum(f.stat().st_size for f in a.iterdir()) <= bench.DUMP_LIMIT_BYTES
    pixels, sample = np.load(a / "image_sample_pixels.npy"), np.load(a / "image_sample.npy")
    assert pixels.dtype == np.float64 and sample.dtype == np.float32
    idx = pixels.astype(np.int64)
    assert np.array_equal(idx, pixels) and np.all(np.diff(idx) > 0) and idx[-1] < 2160 * 3840
    assert np.array_equal(sample, img.reshape(-1, 3)[idx])
    assert np.array_equal(np.load(b / "image_sample_pixels.npy"), pixels)
    assert np.array_equal(np.load(b / "image_sample.npy"), sample)
