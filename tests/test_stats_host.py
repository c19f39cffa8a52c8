"""CPU tests of the sample-statistics surface (include/ptr_stats.h): the exported functions and their ctypes table, the argument
checks, the CLI flag, the oracle-only part of the variance fixture, and self-checks of the numpy restatements the GPU tests compare
the kernels with (tests/stats_ref.py, tests/denoise_cov_ref.py)."""
import ctypes as C
import importlib
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import stats_ref
from denoise_cov_ref import denoise_cov_ref_all, pixel_variance, prefilter

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_library_exports_every_function_of_the_stats_header():
    text = open(os.path.join(ROOT, "include", "ptr_stats.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    counts = {}
    for name, params in re.findall(r"\b(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text):
        counts[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    assert set(counts) == set(pt.STATS_SYMBOLS) and len(counts) == len(pt.STATS_SYMBOLS) == 5
    assert counts == {"ptr_render_bands_cov_device": 12, "ptr_render_bands_cov": 11, "ptr_denoise_cov": 12, "ptr_denoise_cov_device": 11,
                      "ptr_stats_debug_samples": 6}
    lib = pt.load_library()
    for name, count in counts.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count, name
        assert fn.restype is C.c_int, name


def test_stats_symbols_are_in_no_other_table():
    assert not set(pt.STATS_SYMBOLS) & (set(pt.ABI_SYMBOLS) | set(pt.DEBUG_SYMBOLS) | set(pt.POST_SYMBOLS))
    assert len(set(pt.STATS_SYMBOLS)) == len(pt.STATS_SYMBOLS)


# --------------------------------------------------------------------------- bad arguments
def _render_call(name, scene, settings, spp, part, parts, rgb, cov):
    """ptr_render_bands_cov / ptr_render_bands_cov_device / ptr_stats_debug_samples with the given (possibly bad) arguments -> (return
    code, message).  `scene` is a made-up handle: a bad argument must be refused before anything looks behind it."""
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    sp = None if settings is None else C.byref(settings)
    if name == "ptr_render_bands_cov":
        rc = lib.ptr_render_bands_cov(scene, sp, spp, part, parts, fp(rgb), fp(cov), 0, None, err, len(err))
    elif name == "ptr_render_bands_cov_device":
        rc = lib.ptr_render_bands_cov_device(scene, sp, spp, part, parts, vp(rgb), vp(cov), None, 0, None, err, len(err))
    else:
        rc = lib.ptr_stats_debug_samples(scene, sp, spp, fp(rgb), err, len(err))
    return rc, err.value.decode()


@pytest.mark.parametrize("name", ["ptr_render_bands_cov", "ptr_render_bands_cov_device"])
def test_bad_render_arguments_are_refused_by_name(name):
    settings = pt.PtrSettings()
    settings.width, settings.height, settings.maxDepth = 8, 8, 2
    empty = pt.PtrSettings()
    rgb, cov = np.full((8, 8, 3), 7.0, np.float32), np.full((8, 8, 6), 7.0, np.float32)
    scene = C.c_void_p(0x1000)      # never dereferenced by a refused call
    cases = [(None, settings, 4, 0, 1, rgb, cov), (scene, None, 4, 0, 1, rgb, cov), (scene, settings, 4, 0, 1, None, cov),
             (scene, settings, 4, 0, 1, rgb, None),
             (scene, settings, 1, 0, 1, rgb, cov), (scene, settings, 0, 0, 1, rgb, cov),      # a sample covariance needs two samples
             (scene, settings, 4, 0, 0, rgb, cov), (scene, settings, 4, 1, 1, rgb, cov), (scene, settings, 4, 3, 2, rgb, cov),
             (scene, empty, 4, 0, 1, rgb, cov)]
    for case in cases:
        rc, message = _render_call(name, *case)
        assert rc == 1 and message.startswith(name + ":"), (case[2:5], rc, message)
    rc, message = _render_call(name, scene, settings, 1, 0, 1, rgb, cov)
    assert "spp" in message
    assert (rgb == 7.0).all() and (cov == 7.0).all()


def test_bad_debug_samples_arguments_are_refused_by_name():
    settings = pt.PtrSettings()
    settings.width, settings.height = 8, 8
    out = np.full((2, 8, 8, 3), 7.0, np.float32)
    scene = C.c_void_p(0x1000)
    for case in [(None, settings, 2, out), (scene, None, 2, out), (scene, settings, 2, None), (scene, settings, 0, out),
                 (scene, pt.PtrSettings(), 2, out)]:
        rc, message = _render_call("ptr_stats_debug_samples", case[0], case[1], case[2], 0, 1, case[3], None)
        assert rc == 1 and message.startswith("ptr_stats_debug_samples:"), (rc, message)
    assert (out == 7.0).all()


def _denoise_call(name, rgb, albedo, normal, cov, width, height, params, out):
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    pp = None if params is None else C.byref(params)
    if name == "ptr_denoise_cov":
        rc = lib.ptr_denoise_cov(fp(rgb), fp(albedo), fp(normal), fp(cov), width, height, pp, 0, fp(out), None, err, len(err))
    else:
        rc = lib.ptr_denoise_cov_device(vp(rgb), vp(albedo), vp(normal), vp(cov), width, height, pp, vp(out), None, err, len(err))
    return rc, err.value.decode()


def _denoise_inputs():
    return (np.ones((4, 4, 3), np.float32), np.ones((4, 4, 4), np.float32), np.ones((4, 4, 4), np.float32), np.ones((4, 4, 6), np.float32))


@pytest.mark.parametrize("name", ["ptr_denoise_cov", "ptr_denoise_cov_device"])
def test_bad_denoise_arguments_are_refused_by_name(name):
    """the case list of tests/test_post_host.py, plus the covariance pointer"""
    rgb, albedo, normal, cov = _denoise_inputs()
    out = np.full_like(rgb, 7.0)
    good = pt.PtrDenoiseParams.defaults()
    bad_params = [pt.PtrDenoiseParams.defaults(iterations=0), pt.PtrDenoiseParams.defaults(iterations=9)]
    for field in ("sigmaLuminance", "sigmaNormal", "sigmaDepth"):
        bad_params += [pt.PtrDenoiseParams.defaults(**{field: v}) for v in (0.0, -1.0, math.nan, math.inf)]
    cases = [(None, albedo, normal, cov, 4, 4, good, out), (rgb, None, normal, cov, 4, 4, good, out), (rgb, albedo, None, cov, 4, 4, good, out),
             (rgb, albedo, normal, None, 4, 4, good, out), (rgb, albedo, normal, cov, 4, 4, None, out), (rgb, albedo, normal, cov, 4, 4, good, None),
             (rgb, albedo, normal, cov, 0, 4, good, out), (rgb, albedo, normal, cov, 4, 0, good, out)]
    cases += [(rgb, albedo, normal, cov, 4, 4, p, out) for p in bad_params]
    for case in cases:
        rc, message = _denoise_call(name, *case)
        assert rc == 1 and message.startswith(name + ":"), (case[4:7], rc, message)
    assert (out == 7.0).all()


def test_stats_fail_loudly_without_gpu():
    if pt.device_count() > 0:
        pytest.skip("a GPU is present")
    rgb, albedo, normal, cov = _denoise_inputs()
    out = np.full_like(rgb, 7.0)
    for name in ("ptr_denoise_cov", "ptr_denoise_cov_device"):
        rc, message = _denoise_call(name, rgb, albedo, normal, cov, 4, 4, pt.PtrDenoiseParams.defaults(), out)
        assert rc != 0 and "no CPU fallback" in message, (name, rc, message)
    assert (out == 7.0).all()
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.denoise(rgb, albedo, normal, cov=cov)
    host = pt.HostScene.load(os.path.join(GOLDEN, "smoke.scene"))
    with pytest.raises(pt.PtrError, match="no HIP device|no such HIP device"):
        pt.DeviceScene(host.desc).render_image_cov(host.settings_for(width=8, height=8), 4)


def test_cli_documents_and_checks_the_variance_flag():
    helped = subprocess.run([pt.CLI_PATH, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert helped.returncode == 0 and "--denoiseVariance=<spatial|sample>" in helped.stdout
    scene = os.path.join(GOLDEN, "smoke.scene")
    run = lambda *flags: subprocess.run([pt.CLI_PATH, "--scene=" + scene, *flags], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    usage_errors = [("--denoise", "--denoiseVariance=temporal"), ("--denoise", "--denoiseVariance="), ("--denoiseVariance=sample",),
                    ("--denoise=0", "--denoiseVariance=sample"), ("--denoise", "--denoiseVariance=sample", "--sppTotal=1")]
    for flags in usage_errors:
        res = run(*flags)
        assert res.returncode != 0 and "denoiseVariance" in res.stdout and "Usage:" in res.stdout, flags
    for devices in ("--devices=2", "--devices=0"):
        res = run("--denoise", "--denoiseVariance=sample", devices)
        assert res.returncode != 0 and "denoiseVariance=sample" in res.stdout and "device" in res.stdout, devices
        assert "Usage:" not in res.stdout and "HIP" not in res.stdout      # refused with a message, before any device call


# --------------------------------------------------------------------------- the variance fixture: what the oracle alone gives
def test_oracle_only_ratios_of_the_variance_fixture_lie_in_the_band():
    """tests/test_gpu_stats.py asks 0.85 <= (mean over seeds of sum_pixels k^T C k) / S <= 1.15 of the device.  The fixture holds the same
    ratio made from oracle renders alone (tests/golden/make_variance_golden.py): a correct covariance lies in the band with room to spare,
    and the fixture's own noise (S from one half of the seeds against the other) is far below the band's width."""
    fx = json.load(open(os.path.join(GOLDEN, "vectors", "cornell_32x32_d4_4spp_lumvar.json")))
    assert fx["S"] > 0 and fx["spp"] == 4 and len(fx["oracle_ratios"]) == 6
    assert all(0.85 <= r <= 1.15 for r in fx["oracle_ratios"]), fx["oracle_ratios"]
    assert fx["half_difference"] < 0.05
    # the two wrong normalisations at n = 4 - dividing by n^2, and by (n - 1)^2 - would be far outside
    assert 0.75 * max(fx["oracle_ratios"]) < 0.85 and (4.0 / 3.0) * min(fx["oracle_ratios"]) > 1.15


# --------------------------------------------------------------------------- the restatements check themselves and each other
def test_float32_welford_against_the_float64_two_pass():
    """Heavy-tailed synthetic samples (lognormal, 1 % outliers of 1e4, pixels whose samples are all equal), n in {2, 3, 7, 64}: the largest
    |w32 - c64| / sqrt(C_aa C_bb) over all of them is measured here, on the CPU - 1.281e-4, at n = 2 - and the bound the CPU and GPU tests
    assert is four times that (stats_ref.BOUND = 5.124e-4), to cover other inputs.  Samples that are all equal give exactly 0."""
    worst = 0.0
    for n in (2, 3, 7, 64):
        x = stats_ref.heavy_tailed_samples(n)
        w32, c64 = stats_ref.welford32(x), stats_ref.two_pass64(x)
        assert w32.dtype == np.float32 and w32.shape == (x.shape[1], 6) and np.isfinite(w32).all()
        err = stats_ref.relative_error(w32, c64)
        print("welford32 against two_pass64, n = %d: worst relative error %.4e" % (n, err))
        worst = max(worst, err)
        assert (w32[-64:] == 0.0).all() and (c64[-64:] == 0.0).all()      # all-equal samples
        assert (w32[:-64, :3] > 0.0).all()                                 # ... and the others have a variance
    print("worst %.4e, bound %.4e" % (worst, stats_ref.BOUND))
    assert abs(worst - stats_ref.MEASURED_WORST) <= 0.01 * stats_ref.MEASURED_WORST      # the figure the bound is made from
    assert worst <= stats_ref.BOUND


def test_welford_is_the_covariance_of_the_mean():
    """n samples of unit variance and correlation 0.5 between r and g: cov of the mean is (1/n) x that, within sampling noise."""
    rng = np.random.default_rng(3)
    n, pixels = 8, 20000
    z = rng.standard_normal((n, pixels, 3))
    z[..., 1] = 0.5 * z[..., 0] + math.sqrt(0.75) * z[..., 1]
    mean = stats_ref.welford32(z.astype(np.float32)).astype(np.float64).mean(axis=0)
    want = np.array([1.0, 1.0, 1.0, 0.5, 0.0, 0.0]) / n
    assert np.abs(mean - want).max() < 0.01 / n * 5


def _guides(h, w):
    albedo = np.ones((h, w, 4), np.float32)
    normal = np.zeros((h, w, 4), np.float32)
    normal[..., :3] = (0.5, 0.5, 1.0)
    normal[..., 3] = 2.0
    return albedo, normal


def test_constant_variance_stays_constant_through_the_prefilter():
    """A covariance that gives every pixel the same v - with demodulation, C = v0 (a a^T) / (k.1)^2 scaled per pixel by its albedo - gives
    the filter a constant v_p: the prefilter is a weighted MEAN, at the image's corners and beside misses too."""
    rng = np.random.default_rng(9)
    h, w = 7, 9
    albedo, normal = _guides(h, w)
    albedo[..., :3] = rng.uniform(0.2, 0.9, (h, w, 3))
    albedo[2, 3, 3] = 0.0                   # a miss
    v0 = 0.37
    a = albedo[..., :3].astype(np.float64)
    # x = a * s with var(s) = v0 / (sum k)^2: demodulated luminance sum_c k_c x_c / a_c = s * sum k
    ksum = 0.2126 + 0.7152 + 0.0722
    pairs = stats_ref.PAIRS
    cov = np.stack([a[..., i] * a[..., j] for i, j in pairs], axis=2) * (v0 / ksum ** 2)
    rgb = np.ones((h, w, 3), np.float32)
    vp = denoise_cov_ref_all(rgb, albedo, normal, cov, flags=1, dtype=np.float64, return_variance=True)
    hit = albedo[..., 3] > 0.5
    assert np.abs(vp[hit] - v0).max() <= 1e-6 * v0          # (cov passes through float32 on its way in)
    assert (vp[~hit] == 0).all()
    # without demodulation the same covariance gives a v that follows the albedo: not constant
    vp0 = denoise_cov_ref_all(rgb, albedo, normal, cov, flags=0, dtype=np.float64, return_variance=True)
    assert np.ptp(vp0[hit]) > 0.05 * v0


def test_zero_nan_and_negative_entries_count_as_zero():
    T = np.float64
    a = np.ones((1, 4, 3))
    cov = np.zeros((1, 4, 6), np.float32)
    cov[0, 1, :] = np.nan
    cov[0, 2, :3] = -1.0                     # negative definite
    cov[0, 3, :3] = 2.0
    v = pixel_variance(cov, a, T)
    assert (v[0, :3] == 0).all() and abs(v[0, 3] - 2.0 * (0.2126 ** 2 + 0.7152 ** 2 + 0.0722 ** 2)) < 1e-12
    # ... and through the prefilter a zero pixel takes its neighbours' variance: this is what makes the mode usable at 2-4 spp
    hit = np.ones((1, 4), bool)
    vp = prefilter(v, hit, T)
    assert vp[0, 2] > 0 and vp[0, 0] == 0 and np.isfinite(vp).all()
    # the whole filter stays finite on such input, and a zero covariance filters only where colours agree to 1e-6: the image comes back
    rng = np.random.default_rng(4)
    albedo, normal = _guides(5, 6)
    rgb = rng.uniform(0.2, 1.0, (5, 6, 3)).astype(np.float32)
    out = denoise_cov_ref_all(rgb, albedo, normal, np.zeros((5, 6, 6), np.float32), iterations=2, dtype=np.float64)[-1]
    assert np.isfinite(out).all() and np.abs(out - rgb).max() < 1e-3
