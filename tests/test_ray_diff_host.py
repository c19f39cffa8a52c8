"""CPU tests of the first-hit ray differentials (PTR_METAL_RAY_DIFF): the ABI constant and its ctypes mirror, the CLI values that
select the bit, and the restatement the GPU tests compare against (tests/test_gpu_ray_diff.py).  No GPU involved."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ray_diff_constant_and_unchanged_structs():
    assert pt.PTR_METAL_RAY_DIFF == 256
    bits = [pt.PTR_METAL_MEDIA, pt.PTR_METAL_THIN, pt.PTR_METAL_FACE_NORMAL, pt.PTR_METAL_SPECULAR, pt.PTR_METAL_SSS, pt.PTR_METAL_PBR,
            pt.PTR_METAL_CLAMPS, pt.PTR_METAL_ENV_LOD, pt.PTR_METAL_RAY_DIFF]
    assert bits == [1 << k for k in range(9)]
    header = open(os.path.join(ROOT, "include", "ptr_abi.h")).read()
    assert "PTR_METAL_RAY_DIFF = 256u" in header and "Bit 8 (PTR_METAL_RAY_DIFF" in header
    debug = open(os.path.join(ROOT, "include", "ptr_debug.h")).read()
    assert "ptr_debug_first_hit_textures" in debug and "ptr_debug_texture_sample_grad" in debug
    # a new value of an existing field: no ABI struct changes size
    assert C.sizeof(pt.PtrSettings) == 144
    assert C.sizeof(pt.PtrSceneDesc) == 80
    assert C.sizeof(pt.PtrMaterial) == 576


def test_cli_accepts_the_ray_diff_semantics_and_rejects_junk():
    exe = pt.CLI_PATH
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "metal-raydiff" in r.stdout and "metal-envlod-raydiff" in r.stdout
    for flags in (["--semantics=metal-raydiff"], ["--semantics", "metal-raydiff"], ["--semantics=metal-envlod-raydiff"],
                  ["--backend=metal", "--semantics=metal-raydiff"], ["--semantics=metal-envlod"], ["--semantics=metal"]):
        r = subprocess.run([exe, "--scene=/nonexistent.scene"] + flags, capture_output=True, text=True)
        assert r.returncode == 1 and "Failed to load scene" in r.stderr and "Invalid value" not in r.stderr, flags
    for junk in ("metal-raydif", "raydiff", "metal-raydiff-envlod", "metal+raydiff"):
        r = subprocess.run([exe, "--scene=x.scene", "--semantics=" + junk], capture_output=True, text=True)
        assert r.returncode == 1 and "Invalid value for --semantics" in r.stderr, junk


def igehy_dpdx(cam_origin, lower_left, horizontal, vertical, width, height, D, t, N):
    """The restatement in float64 (include/ptr_abi.h bit 8): dPdx, dPdy of a hit at world distance t along the unit direction D."""
    c = np.cross(horizontal, vertical)
    dlen = np.dot(lower_left - cam_origin, c) / np.dot(D, c)
    ddx, ddy = horizontal / width, -vertical / height
    s = t / dlen
    nd = np.dot(N, D)
    return s * (ddx - np.dot(N, ddx) / nd * D), s * (ddy - np.dot(N, ddy) / nd * D)


def test_restated_differentials_match_neighbouring_pixels():
    """Check the restatement itself against finite differences.  Trace the rays of pixel positions (x, y), (x + e, y) and (x, y + e) from
    one lens point to a tilted plane.  The hit points then differ by e dPdx and e dPdy to first order: the unnormalised direction is
    linear in the pixel position, and the lens offset lies in the image plane, so it shifts |d| but not the plane's depth."""
    rng = np.random.default_rng(5)
    origin = np.array([0.3, 1.2, 4.0])
    w_axis = np.array([0.1, 0.25, 1.0]) / np.linalg.norm([0.1, 0.25, 1.0])
    u_axis = np.cross([0.0, 1.0, 0.0], w_axis)
    u_axis /= np.linalg.norm(u_axis)
    v_axis = np.cross(w_axis, u_axis)
    width, height, focus = 64.0, 48.0, 3.5
    horizontal, vertical = 2.0 * focus * u_axis, 1.5 * focus * v_axis
    lower_left = origin - 0.5 * horizontal - 0.5 * vertical - focus * w_axis
    N = np.array([0.05, 1.0, -0.2]) / np.linalg.norm([0.05, 1.0, -0.2])
    plane_d = -0.4

    def hit(px, py, lens):
        o = origin + lens[0] * u_axis + lens[1] * v_axis
        d = lower_left + (px / width) * horizontal + (1.0 - py / height) * vertical - o
        D = d / np.linalg.norm(d)
        t = (plane_d - np.dot(N, o)) / np.dot(N, D)
        return o + t * D, D, t

    e = 1e-4
    for _ in range(20):
        px, py = rng.uniform(4, 60), rng.uniform(30, 46)
        lens = rng.uniform(-0.05, 0.05, 2)
        p, D, t = hit(px, py, lens)
        assert t > 0
        dpdx, dpdy = igehy_dpdx(origin, lower_left, horizontal, vertical, width, height, D, t, N)
        fx = (hit(px + e, py, lens)[0] - p) / e
        fy = (hit(px, py + e, lens)[0] - p) / e
        assert np.allclose(dpdx, fx, rtol=1e-3, atol=1e-6 * np.abs(fx).max())
        assert np.allclose(dpdy, fy, rtol=1e-3, atol=1e-6 * np.abs(fy).max())
