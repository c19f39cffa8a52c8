"""GPU tests of the per-pixel sample covariance (include/ptr_stats.h, csrc/kernels/stats.hip) and of the denoiser run on it
(k_denoise_prepare_cov in csrc/kernels/denoise.hip), against their numpy restatements (tests/stats_ref.py, tests/denoise_cov_ref.py),
against the oracle's across-seed variance (tests/golden/make_variance_golden.py) and against the invariances the header promises.

The scene is tests/golden/cornell_small_mesh.scene at depth 4."""
import functools
import importlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import stats_ref
from denoise_cov_ref import denoise_cov_ref_all
from test_gpu_denoise import make_inputs, params

pt = importlib.import_module("metal-pathtracer-arm64_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(ROOT, "scenes")
LUMA = np.array([0.2126, 0.7152, 0.0722])


def open_scene():
    host = pt.HostScene.load(os.path.join(GOLDEN, "cornell_small_mesh.scene"), SCENES)
    return host, pt.DeviceScene(host.desc, 0, keepalive=host)


@pytest.fixture(scope="module")
def cornell():
    return open_scene()


# --------------------------------------------------------------------------- 1. the covariance is the header's recurrence
@pytest.mark.parametrize("spp", [2, 5, 16])
def test_cov_is_the_float32_welford_of_the_samples(cornell, spp):
    """37x21: three bands, the last of five rows, and ragged 8x8 pixel blocks."""
    host, dev = cornell
    w, h = 37, 21
    s = host.settings_for(width=w, height=h, max_depth=4, seed=1337)
    image, _ = dev.render_image(s, spp)
    rgb_bands, cov_bands, stats = dev.render_cov(s, spp)
    assert rgb_bands.shape == (24, w, 3) and cov_bands.shape == (24, w, 6) and stats.samples == w * h * spp
    assert np.array_equal(rgb_bands[:h], image)                                   # the image did not move
    assert (cov_bands[h:] == 0.0).all() and (rgb_bands[h:] == 0.0).all()          # padding rows
    rgb2, cov, _ = dev.render_image_cov(s, spp)
    assert np.array_equal(rgb2, image) and np.array_equal(cov, cov_bands[:h])
    samples = dev.debug_samples(s, spp)
    assert samples.shape == (spp, h, w, 3)
    # the probe returns what k_resolve sums: their float32 sum in sample order, divided by spp, is the image
    total = np.zeros((h, w, 3), np.float32)
    for c in range(spp):
        total = total + samples[c]
    assert np.array_equal(total / np.float32(spp), image)
    want = stats_ref.welford32(samples)
    assert cov.dtype == np.float32 and np.isfinite(cov).all()
    assert np.array_equal(cov, want), "largest difference %.3e" % float(np.abs(cov - want).max())
    c64 = stats_ref.two_pass64(samples)
    err = stats_ref.relative_error(cov, c64)
    print("cov against the float64 two-pass, %d spp: worst relative error %.3e (bound %.3e)" % (spp, err, stats_ref.BOUND))
    assert err <= stats_ref.BOUND
    assert (cov[..., :3] >= 0.0).all() and (cov[..., :3] > 0.0).mean() > 0.1      # variances; not a buffer of zeros
    flat = (c64[..., 0] == 0) & (c64[..., 1] == 0) & (c64[..., 2] == 0)
    assert (cov[flat] == 0.0).all()


# --------------------------------------------------------------------------- 2. invariance
def test_cov_does_not_depend_on_how_the_frame_is_rendered(cornell):
    host, dev = cornell
    w, h, spp = 37, 21, 7
    s = host.settings_for(width=w, height=h, max_depth=4, seed=1337)
    image, base, _ = dev.render_image_cov(s, spp)
    assert np.array_equal(dev.render_image_cov(s, spp)[1], base)                  # two runs
    assert np.array_equal(base, stats_ref.welford32(dev.debug_samples(s, spp)))
    for parts in (1, 2, 3):
        outs = [dev.render_cov(s, spp, p, parts) for p in range(parts)]
        assert np.array_equal(pt.assemble_bands([o[1] for o in outs], w, h), base), parts
        assert np.array_equal(pt.assemble_bands([o[0] for o in outs], w, h), image), parts

    def with_env(env, fresh_scene):
        os.environ.update(env)
        try:
            scene = open_scene()[1] if fresh_scene else dev       # the pool knobs are read when a scene is uploaded
            rgb, cov, _ = scene.render_image_cov(s, spp)
            plain, _ = scene.render_image(s, spp)
            if fresh_scene:
                scene.close()
        finally:
            for k in env:
                del os.environ[k]
        assert np.array_equal(rgb, plain), env                     # (a frame of several passes sums in another order than one pass)
        return cov

    # PTR_MAX_ITEMS: 2331 = three samples per pixel and pass (passes of 3, 3 and 1 samples), 777 = one (seven passes)
    for env, fresh in (({"PTR_MAX_ITEMS": "2331"}, False), ({"PTR_MAX_ITEMS": "777"}, False), ({"PTR_POOL_SLOTS": "1024"}, True),
                       ({"PTR_POOL_GROUPS": "1"}, True), ({"PTR_MAX_ITEMS": "2331", "PTR_POOL_SLOTS": "1024"}, True)):
        assert np.array_equal(with_env(env, fresh), base), env
    os.environ["PTR_MAX_ITEMS"] = "2331"
    try:
        outs = [dev.render_cov(s, spp, p, 2)[1] for p in range(2)]                # passes x partitions
        with pytest.raises(pt.PtrError, match="more than one pass"):
            dev.debug_samples(s, spp)
    finally:
        del os.environ["PTR_MAX_ITEMS"]
    assert np.array_equal(pt.assemble_bands(outs, w, h), base)
    # the device entry point on a stream of torch's
    t_rgb = torch.full((24, w, 3), 7.0, device="cuda")
    t_cov = torch.full((24, w, 6), 7.0, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.render_cov_device(s, spp, t_rgb.data_ptr(), t_cov.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(t_cov.cpu().numpy()[:h], base) and np.array_equal(t_rgb.cpu().numpy()[:h], image)
    assert (t_cov.cpu().numpy()[h:] == 0.0).all()
    with pytest.raises(pt.PtrError, match="ptr_render_bands_cov: .*spp"):
        dev.render_image_cov(s, 1)


# --------------------------------------------------------------------------- 3. the statistic means what it says
def test_cov_adds_up_to_the_variance_across_seeds(cornell):
    """32x32, 4 spp, seeds 1..128: sum over pixels of k^T C k (k the luminance weights), averaged over the seeds, against the oracle's
    across-seed variance of the image's luminance summed over the pixels (S of tests/golden/vectors/cornell_32x32_d4_4spp_lumvar.json,
    made from 256 oracle renders).  In expectation the two are equal.  Condition: 0.85 <= ratio <= 1.15 - the wrong normalisations at
    n = 4, dividing by n^2 or by (n - 1)^2, give 0.75 and 1.33; the oracle alone, fed through the same formula, gives 0.946 .. 0.981 and
    S differs by 2.5 % between its two halves (tests/test_stats_host.py holds the fixture to that)."""
    host, dev = cornell
    fx = json.load(open(os.path.join(GOLDEN, "vectors", "cornell_32x32_d4_4spp_lumvar.json")))
    k = np.array(fx["luma"])
    sums = []
    for seed in range(1, 129):
        s = host.settings_for(width=fx["width"], height=fx["height"], max_depth=fx["depth"], seed=seed)
        cov = dev.render_image_cov(s, fx["spp"])[1].astype(np.float64)
        quad = (k[0] * k[0] * cov[..., 0] + k[1] * k[1] * cov[..., 1] + k[2] * k[2] * cov[..., 2]
                + 2.0 * (k[0] * k[1] * cov[..., 3] + k[0] * k[2] * cov[..., 4] + k[1] * k[2] * cov[..., 5]))
        sums.append(float(quad.sum()))
    ratio = float(np.mean(sums)) / fx["S"]
    print("sum_pixels k^T C k over 128 seeds / S = %.4f (oracle alone: %s)" % (ratio, ", ".join("%.3f" % r for r in fx["oracle_ratios"])))
    assert 0.85 <= ratio <= 1.15


# --------------------------------------------------------------------------- 4. the denoiser on a covariance
def make_cov(w, h, rgb, seed=13):
    """a random symmetric positive-definite covariance per pixel, of the size a few samples of `rgb` would have, plus pixels that are
    zero, NaN and indefinite"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((h, w, 3, 3))
    spd = a @ np.swapaxes(a, 2, 3) + 0.1 * np.eye(3)
    scale = (0.3 * rgb.astype(np.float64).mean(axis=2)) ** 2
    spd = spd * scale[..., None, None]
    cov = np.stack([spd[..., i, j] for i, j in stats_ref.PAIRS], axis=2).astype(np.float32)
    kind = rng.integers(0, 12, (h, w))
    cov[kind == 0] = 0.0
    cov[kind == 1] = np.nan
    cov[kind == 2] = cov[kind == 2] * np.float32(-1.0)      # negative definite
    cov[kind == 3, :3] = 0.0                                # no variances, only covariances: indefinite
    return cov


COV_SIZES = [(1, 1), (5, 3), (67, 45)]


@functools.lru_cache(maxsize=None)
def cov_references(w, h, flags):
    """(inputs, float64 restatement, float32 restatement) for 1..5 passes: computed once, shared by the cases, never written to"""
    rgb, albedo, normal = make_inputs(w, h)
    inputs = (rgb, albedo, normal, make_cov(w, h, rgb))
    ref64 = denoise_cov_ref_all(*inputs, iterations=5, flags=flags, dtype=np.float64)
    ref32 = denoise_cov_ref_all(*inputs, iterations=5, flags=flags, dtype=np.float32)
    for a in inputs + tuple(ref64) + tuple(ref32):
        a.setflags(write=False)
    return inputs, ref64, ref32


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("size", COV_SIZES, ids=lambda s: "%dx%d" % s)
def test_denoise_cov_parity_with_the_float64_restatement(size, iterations, flags):
    """The rule of tests/test_gpu_denoise.py: every pixel within tol = max(8 x max|ref32 - ref64|, 1e-5 x max|ref64|) of the float64
    restatement; the tolerance comes from the two restatements alone."""
    w, h = size
    inputs, ref64, ref32 = cov_references(w, h, flags)
    rgb, albedo, normal, cov = inputs
    want = ref64[iterations - 1]
    tol = max(8.0 * float(np.abs(ref32[iterations - 1].astype(np.float64) - want).max()), 1e-5 * float(np.abs(want).max()))
    got = pt.denoise(rgb, albedo, normal, params=params(iterations=iterations, flags=flags), cov=cov)
    assert got.shape == (h, w, 3) and got.dtype == np.float32 and np.isfinite(got).all()
    worst = float(np.abs(got.astype(np.float64) - want).max())
    print("denoise-cov parity %dx%d iterations %d flags %d: max|gpu - ref64| = %.3e, tol = %.3e, ratio %.4f"
          % (w, h, iterations, flags, worst, tol, worst / tol))
    assert worst <= tol
    miss = albedo[..., 3] < 0.5
    assert np.array_equal(got[miss], rgb[miss])                                   # miss pixels pass through
    if w * h > 15:
        assert float(np.abs(got - rgb).max()) > 10 * tol                          # (and the filter moved the image by far more than that)
        spatial = pt.denoise(rgb, albedo, normal, params=params(iterations=iterations, flags=flags))
        assert not np.array_equal(spatial, got)                                   # ... and not to where the spatial variance moves it


def test_denoise_cov_gives_the_same_bits_on_every_path():
    for w, h in ((67, 45), (5, 3)):
        inputs, _, _ = cov_references(w, h, 1)
        rgb, albedo, normal, cov = inputs
        p = params()
        before = pt.denoise(rgb, albedo, normal, params=p)
        host = pt.denoise(rgb, albedo, normal, params=p, cov=cov)
        assert np.array_equal(pt.denoise(rgb, albedo, normal, params=p, cov=cov), host)
        t_rgb, t_albedo, t_normal, t_cov = (torch.from_numpy(a.copy()).cuda() for a in (rgb, albedo, normal, cov))
        t_io = t_rgb.clone()
        pt.denoise_device(t_io.data_ptr(), t_albedo.data_ptr(), t_normal.data_ptr(), w, h, params=p, d_cov=t_cov.data_ptr(),
                          stream=torch.cuda.current_stream().cuda_stream)            # in place
        torch.cuda.synchronize()
        assert np.array_equal(t_io.cpu().numpy(), host)
        t_out = torch.zeros_like(t_rgb)
        pt.denoise_device(t_rgb.data_ptr(), t_albedo.data_ptr(), t_normal.data_ptr(), w, h, params=p, d_out=t_out.data_ptr(), d_cov=t_cov.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(t_out.cpu().numpy(), host) and np.array_equal(t_rgb.cpu().numpy(), rgb)
        assert np.array_equal(t_cov.cpu().numpy(), cov, equal_nan=True)            # the covariance is an input only
        try:
            for knob in ("0", "1"):      # the passes behind the new prepare, through the caches / staged in LDS
                os.environ["PTR_DENOISE_TILED"] = knob
                assert np.array_equal(pt.denoise(rgb, albedo, normal, params=p, cov=cov), host), (w, h, knob)
        finally:
            del os.environ["PTR_DENOISE_TILED"]
        # the calls without a covariance are today's
        assert np.array_equal(pt.denoise(rgb, albedo, normal, params=p, cov=None), before)
        t_io = t_rgb.clone()
        pt.denoise_device(t_io.data_ptr(), t_albedo.data_ptr(), t_normal.data_ptr(), w, h, params=p, d_cov=0)
        torch.cuda.synchronize()
        assert np.array_equal(t_io.cpu().numpy(), before)


# --------------------------------------------------------------------------- 5. end to end, and the CLI
@pytest.fixture(scope="module")
def cornell_4spp(cornell):
    host, dev = cornell
    s = host.settings_for(width=64, height=64, max_depth=4, seed=1337)
    img, cov, _ = dev.render_image_cov(s, 4)
    albedo, normal = dev.render_aovs(s, 0)
    return img, cov, albedo, normal


def test_it_denoises_on_the_measured_variance(cornell_4spp):
    """4 spp, denoised on its own sample variance, is nearer the 32-spp golden than before.  Which of the two variances serves better is a
    measurement (printed), not a condition."""
    img, cov, albedo, normal = cornell_4spp
    golden = pt.read_pfm(os.path.join(GOLDEN, "vectors", "cornell_64x64_d4_32spp_seed1337.pfm"))
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - golden.astype(np.float64)) ** 2)))
    spatial = pt.denoise(img, albedo, normal)
    sample = pt.denoise(img, albedo, normal, cov=cov)
    print("cornell 64x64 4 spp vs 32 spp golden, RMSE: raw %.5f, spatial variance %.5f, sample variance %.5f" % (rmse(img), rmse(spatial), rmse(sample)))
    assert np.isfinite(sample).all() and rmse(sample) < rmse(img)


def test_cli_denoise_variance(cornell_4spp, tmp_path):
    img, cov, albedo, normal = cornell_4spp
    common = [pt.CLI_PATH, "--scene=" + os.path.join(GOLDEN, "cornell_small_mesh.scene"), "--assets=" + SCENES, "--width=64", "--height=64",
              "--sppTotal=4", "--maxDepth=4", "--seed=1337", "--format=pfm", "--denoise"]
    plain, spatial, sample = tmp_path / "plain.pfm", tmp_path / "spatial.pfm", tmp_path / "sample.pfm"
    r = subprocess.run(common + ["--output=" + str(plain), "--verbose"], capture_output=True, text=True)
    assert r.returncode == 0 and "variance from the 7x7 spatial estimate" in r.stderr, r.stderr
    assert np.array_equal(pt.read_pfm(str(plain)), pt.denoise(img, albedo, normal))
    r = subprocess.run(common + ["--output=" + str(spatial), "--denoiseVariance=spatial"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert spatial.read_bytes() == plain.read_bytes()
    r = subprocess.run(common + ["--output=" + str(sample), "--denoiseVariance=sample", "--verbose"], capture_output=True, text=True)
    assert r.returncode == 0 and "variance from the per-pixel sample covariance" in r.stderr, r.stderr
    assert np.array_equal(pt.read_pfm(str(sample)), pt.denoise(img, albedo, normal, cov=cov))
    assert sample.read_bytes() != plain.read_bytes()
