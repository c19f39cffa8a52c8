"""CPU tests of the denoiser's surface (include/ptr_post.h): the exported functions and their ctypes table, the argument checks, the CLI
flags, and self-checks of the numpy restatement the GPU tests compare the kernels with (tests/denoise_ref.py)."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

from denoise_ref import B3, denoise_ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_function_of_the_post_header():
    text = open(os.path.join(ROOT, "include", "ptr_post.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    counts = {}
    for name, params in re.findall(r"\b(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text):
        counts[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    assert set(counts) == set(pt.POST_SYMBOLS) and len(counts) == len(pt.POST_SYMBOLS) == 4
    assert {"ptr_denoise_default_params", "ptr_denoise", "ptr_denoise_device"} <= set(counts)
    assert not set(pt.POST_SYMBOLS) & (set(pt.ABI_SYMBOLS) | set(pt.DEBUG_SYMBOLS))
    lib = pt.load_library()
    for name, count in counts.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count, name
        assert fn.restype is (None if name == "ptr_denoise_default_params" else C.c_int), name
    # the ctypes mirror of PtrDenoiseParams: five 4-byte fields in the header's order
    fields = re.search(r"typedef struct PtrDenoiseParams \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [name for name, _ in pt.PtrDenoiseParams._fields_]
    assert C.sizeof(pt.PtrDenoiseParams) == 20


def test_default_params():
    p = pt.PtrDenoiseParams(9, 9.0, 9.0, 9.0, 9)
    pt.load_library().ptr_denoise_default_params(C.byref(p))
    assert (p.iterations, p.sigmaLuminance, p.sigmaNormal, p.sigmaDepth, p.flags) == (5, 4.0, 128.0, 1.0, 1)
    q = pt.PtrDenoiseParams.defaults(iterations=3)
    assert (q.iterations, q.sigmaNormal, q.flags) == (3, 128.0, pt.PTR_DENOISE_DEMODULATE)


def _call(name, rgb, albedo, normal, width, height, params, out):
    """ptr_denoise / ptr_denoise_device / ptr_denoise_timed with the given (possibly bad) arguments -> (return code, message).  The
    pointers are host arrays: a bad argument must be refused before any device call looks at them."""
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    pp = None if params is None else C.byref(params)
    if name == "ptr_denoise":
        rc = lib.ptr_denoise(fp(rgb), fp(albedo), fp(normal), width, height, pp, 0, fp(out), None, err, len(err))
    elif name == "ptr_denoise_device":
        rc = lib.ptr_denoise_device(vp(rgb), vp(albedo), vp(normal), width, height, pp, vp(out), None, err, len(err))
    else:
        ms = (C.c_double * 10)()
        rc = lib.ptr_denoise_timed(vp(rgb), vp(albedo), vp(normal), width, height, pp, vp(out), 1, 0, ms, None, err, len(err))
    return rc, err.value.decode()


@pytest.mark.parametrize("name", ["ptr_denoise", "ptr_denoise_device", "ptr_denoise_timed"])
def test_bad_arguments_are_refused_by_name(name):
    rgb, albedo, normal = np.ones((4, 4, 3), np.float32), np.ones((4, 4, 4), np.float32), np.ones((4, 4, 4), np.float32)
    out = np.full_like(rgb, 7.0)
    good = pt.PtrDenoiseParams.defaults()
    bad_params = [pt.PtrDenoiseParams.defaults(iterations=0), pt.PtrDenoiseParams.defaults(iterations=9)]
    for field in ("sigmaLuminance", "sigmaNormal", "sigmaDepth"):
        bad_params += [pt.PtrDenoiseParams.defaults(**{field: v}) for v in (0.0, -1.0, math.nan, math.inf)]
    cases = [(None, albedo, normal, 4, 4, good, out), (rgb, None, normal, 4, 4, good, out), (rgb, albedo, None, 4, 4, good, out),
             (rgb, albedo, normal, 4, 4, None, out), (rgb, albedo, normal, 4, 4, good, None),
             (rgb, albedo, normal, 0, 4, good, out), (rgb, albedo, normal, 4, 0, good, out)]
    cases += [(rgb, albedo, normal, 4, 4, p, out) for p in bad_params]
    for case in cases:
        rc, message = _call(name, *case)
        assert rc == 1 and message.startswith(name + ":"), (case[3:6], rc, message)
    assert (out == 7.0).all()


def test_denoise_fails_loudly_without_gpu():
    if pt.device_count() > 0:
        pytest.skip("a GPU is present")
    rgb, albedo, normal = np.ones((4, 4, 3), np.float32), np.ones((4, 4, 4), np.float32), np.ones((4, 4, 4), np.float32)
    out = np.full_like(rgb, 7.0)
    for name in ("ptr_denoise", "ptr_denoise_device", "ptr_denoise_timed"):
        rc, message = _call(name, rgb, albedo, normal, 4, 4, pt.PtrDenoiseParams.defaults(), out)
        assert rc != 0 and "no CPU fallback" in message, (name, rc, message)
    assert (out == 7.0).all()
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.denoise(rgb, albedo, normal)


def test_cli_documents_and_checks_the_denoise_flags():
    helped = subprocess.run([pt.CLI_PATH, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert helped.returncode == 0
    assert "--denoise[=0|1]" in helped.stdout and "--denoiseIterations=<1..8>" in helped.stdout
    scene = os.path.join(ROOT, "tests", "golden", "smoke.scene")
    for bad in ("--denoise=2", "--denoiseIterations=0", "--denoiseIterations=9", "--denoiseIterations=x"):
        res = subprocess.run([pt.CLI_PATH, "--scene=" + scene, bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode != 0 and "denoise" in res.stdout and "Usage:" in res.stdout, bad


# --------------------------------------------------------------------------- the restatement checks itself (9x7, float64)
def _guides(h, w, rng, flat):
    albedo = np.ones((h, w, 4), np.float32)
    normal = np.zeros((h, w, 4), np.float32)
    if flat:
        normal[..., :3] = (0.5, 0.5, 1.0)   # n = (0, 0, 1)
        normal[..., 3] = 2.0
    else:
        albedo[..., :3] = rng.uniform(0.2, 0.9, (h, w, 3))
        n = rng.normal(size=(h, w, 3))
        normal[..., :3] = n / np.linalg.norm(n, axis=2, keepdims=True) * 0.5 + 0.5
        normal[..., 3] = rng.uniform(1.0, 3.0, (h, w))
        albedo[2, 3, 3] = 0.0               # a miss
    return albedo, normal


def test_restatement_constant_colour_is_a_fixed_point():
    rng = np.random.default_rng(5)
    albedo, normal = _guides(7, 9, rng, flat=False)
    rgb = np.empty((7, 9, 3), np.float32)
    rgb[...] = (0.25, 0.5, 0.125)
    out = denoise_ref(rgb, albedo, normal, flags=0, dtype=np.float64)     # (demodulated, the colour would follow the albedo)
    assert np.abs(out - rgb).max() <= 1e-14
    albedo[..., :3] = (0.5, 0.25, 0.75)
    out = denoise_ref(rgb, albedo, normal, flags=1, dtype=np.float64)
    assert np.abs(out - rgb).max() <= 1e-14


def test_restatement_with_equal_weights_is_the_b3_filter():
    # flat guides (wn = wz = 1) and colours of one luminance (wl = 1): one pass is the 5x5 B3 kernel over the in-image taps, renormalised.
    # The third channel is solved for a luminance of 2^-20 and rounded to float32, which leaves luminance differences below
    # 0.0722 * 2^-24 * |b| < 1e-13 against the 1e-6 in wl's denominator: every wl is within 1e-7 of 1, the result within 1e-6 (relative).
    rng = np.random.default_rng(6)
    h, w = 7, 9
    albedo, normal = _guides(h, w, rng, flat=True)
    rgb = np.empty((h, w, 3), np.float64)
    rgb[..., 0] = rng.uniform(0.1, 0.9, (h, w))
    rgb[..., 1] = rng.uniform(0.1, 0.9, (h, w))
    rgb[..., 2] = (1.0 - 0.2126 * rgb[..., 0] - 0.7152 * rgb[..., 1]) / 0.0722
    rgb = (rgb * 2.0 ** -20).astype(np.float32)
    assert np.ptp(rgb[..., 0]) > 0.5 * 2.0 ** -20
    out = denoise_ref(rgb, albedo, normal, iterations=1, flags=0, dtype=np.float64)
    want = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            total = 0.0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if 0 <= y + dy < h and 0 <= x + dx < w:
                        k = B3[dy + 2] * B3[dx + 2]
                        total += k
                        want[y, x] += k * rgb[y + dy, x + dx].astype(np.float64)
            want[y, x] /= total
    assert np.abs(out - want).max() <= 1e-6 * np.abs(want).max()
    assert np.abs(want - rgb).max() > 0.05 * np.abs(want).max()      # (the filter did something)
