"""GPU tests of HipHeadlessRenderer::render (csrc/host/headless.cpp) through the CLI: one process per frame kind - whole, bands, multi,
adaptive, snapshots - combined with the feature buffers, the denoiser and both sources of its variance.  Every written file equals,
bit for bit, the composition of the same C-ABI calls through the Python package."""
import importlib
import os
import subprocess

import numpy as np
import pytest

pt = importlib.import_module("metal-pathtracer-arm64_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "smoke.scene")
W, H = 64, 48
BVH_LINE = "[ptr] BVH"

ADAPTIVE = ["--sppTotal=8", "--adaptive=0.05", "--adaptiveMinSpp=4", "--adaptiveStep=2", "--aovExr"]
SNAPSHOTS = ["--sppTotal=8", "--snapshots=2,4", "--aovExr"]
SAMPLE = ["--denoise", "--denoiseVariance=sample"]
# name, frame kind, frame flags, what is combined with them
CASES = [
    ("whole", "whole", ["--sppTotal=4"], []),
    ("bands-denoise", "bands", ["--sppTotal=4", "--aovExr"], ["--denoise"]),
    ("bands-denoise-sample", "bands", ["--sppTotal=4", "--aovExr"], SAMPLE),
    ("multi-denoise", "multi", ["--sppTotal=4", "--devices=0", "--aovExr"], ["--denoise"]),
    ("adaptive-denoise", "adaptive", ADAPTIVE, ["--denoise"]),
    ("adaptive-denoise-sample", "adaptive", ADAPTIVE, SAMPLE),
    ("snapshots-denoise", "snapshots", SNAPSHOTS, ["--denoise"]),
    ("snapshots-denoise-sample", "snapshots", SNAPSHOTS, SAMPLE),
]


@pytest.fixture(scope="module")
def smoke():
    """The scene on device 0, the settings of every case and the first-hit feature buffers, computed once."""
    host = pt.HostScene.load(SCENE)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for(width=W, height=H, seed=1337)
    albedo, normal = dev.render_aovs(s, 0)
    return host, dev, s, albedo, normal


def _frame(kind, host, dev, s, want_cov):
    """The frame call of `kind` through the package: (image, covariance or None, {spp: snapshot})."""
    if kind in ("whole", "bands"):
        if want_cov:
            rgb, cov, _ = dev.render_image_cov(s, 4)
            return rgb, cov, {}
        return dev.render_image(s, 4)[0], None, {}
    if kind == "multi":
        return pt.render_multi(host.desc, s, 4, n_devices=0)[0], None, {}
    if kind == "adaptive":
        rgb, cov, _, _, _ = dev.render_adaptive(s, pt.PtrAdaptiveParams(4, 8, 2, 0.05), want_cov=want_cov)
        return rgb, cov, {}
    frame = dev.frame(s)
    snaps, done = {}, 0
    for stop in (2, 4):
        frame.accumulate(stop - done)
        done = stop
        snaps[stop] = frame.resolve(want_cov=False, want_count=False)[0]
    frame.accumulate(8 - done)
    rgb, cov, _ = frame.resolve(want_cov=want_cov, want_count=False)
    frame.close()
    return rgb, cov, snaps


def _exr_planes(path):
    """The ten float planes of the feature EXR per row: B G R, albedo B G R, depth, normal X Y Z (test_cli_devices_and_aov_export)."""
    data = path.read_bytes()
    body = np.frombuffer(data[-(H * (8 + 10 * W * 4)):], np.uint8).reshape(H, 8 + 10 * W * 4)
    return body[:, 8:].copy().view(np.float32).reshape(H, 10, W)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cli_frame_kinds_match_the_package(smoke, tmp_path, case):
    _, kind, frame_flags, combined = case
    host, dev, s, albedo, normal = smoke
    denoise, sample = "--denoise" in combined, "--denoiseVariance=sample" in combined
    rgb, cov, snaps = _frame(kind, host, dev, s, sample)
    want = pt.denoise(rgb, albedo, normal, cov=cov) if denoise else rgb

    out, aov = tmp_path / "frame.pfm", tmp_path / "features.exr"
    flags = [f + "=" + str(aov) if f == "--aovExr" else f for f in frame_flags] + combined
    r = subprocess.run([pt.CLI_PATH, "--scene=" + SCENE, "--width=%d" % W, "--height=%d" % H, "--seed=1337", "--backend=embree", "--format=pfm",
                        "--output=" + str(out), "--verbose"] + flags, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (BVH_LINE in r.stderr) == (kind == "whole"), r.stderr
    assert np.array_equal(pt.read_pfm(str(out)), want)
    files = {"frame.pfm"}
    if "--aovExr" in frame_flags:
        files.add("features.exr")
        planes = _exr_planes(aov)
        hit = albedo[..., 3] > 0.5
        for k in range(3):
            assert np.array_equal(planes[:, 2 - k], want[..., k]), k
            assert np.array_equal(planes[:, 5 - k], albedo[..., k]), k
            assert np.array_equal(planes[:, 7 + k], np.where(hit, normal[..., k] * np.float32(2.0) - np.float32(1.0), np.float32(0.0))), k
        assert np.array_equal(planes[:, 6], normal[..., 3])
    for n, snap in snaps.items():
        files.add("frame.%d.pfm" % n)
        assert np.array_equal(pt.read_pfm(str(tmp_path / ("frame.%d.pfm" % n))), snap), n
    assert {p.name for p in tmp_path.iterdir()} == files
