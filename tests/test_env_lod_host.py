"""CPU tests of the prefiltered environment lookups (PTR_METAL_ENV_LOD): the mip chain the host builds, the ABI constant and
the CLI value that selects the bit.  No GPU involved."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mip_chain(rgba):
    """Restatement of the chain rule of the material textures (csrc/host/hip_backend.cpp appendTextureWithMips): level l + 1 halves both
    sizes (at least 1) and averages the 2x2 block under each texel, the second tap clamped at odd sizes, ((a + b) + (c + d)) * 0.25 in
    float32; down to 1x1."""
    levels = [np.asarray(rgba, dtype=np.float32)]
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        src = levels[-1]
        h, w = src.shape[:2]
        nh, nw = max(h // 2, 1), max(w // 2, 1)
        y0 = np.minimum(2 * np.arange(nh), h - 1)
        y1 = np.minimum(2 * np.arange(nh) + 1, h - 1)
        x0 = np.minimum(2 * np.arange(nw), w - 1)
        x1 = np.minimum(2 * np.arange(nw) + 1, w - 1)
        a, b = src[y0][:, x0], src[y0][:, x1]
        c, d = src[y1][:, x0], src[y1][:, x1]
        levels.append(((a + b) + (c + d)) * np.float32(0.25))
    return levels


@pytest.mark.parametrize("w,h", [(64, 32), (96, 48), (37, 19), (1, 7), (1, 1)])
def test_env_mip_chain_matches_the_texture_rule(w, h):
    rng = np.random.default_rng(w * 131 + h)
    rgba = rng.uniform(0.0, 4.0, size=(h, w, 4)).astype(np.float32)
    chain = pt.debug_env_mips(rgba)
    assert len(chain) == int(np.floor(np.log2(max(w, h)))) + 1
    ref = mip_chain(rgba)
    assert len(chain) == len(ref)
    for got, want in zip(chain, ref):
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # bit for bit
    assert chain[-1].shape[:2] == (1, 1)


def test_env_lod_constant_and_unchanged_structs():
    assert pt.PTR_METAL_ENV_LOD == 128
    bits = [pt.PTR_METAL_MEDIA, pt.PTR_METAL_THIN, pt.PTR_METAL_FACE_NORMAL, pt.PTR_METAL_SPECULAR, pt.PTR_METAL_SSS, pt.PTR_METAL_PBR,
            pt.PTR_METAL_CLAMPS, pt.PTR_METAL_ENV_LOD]
    assert bits == [1 << k for k in range(8)]
    header = open(os.path.join(ROOT, "include", "ptr_abi.h")).read()
    assert "PTR_METAL_ENV_LOD = 128u" in header
    # the bit is a new value of an existing field: no ABI struct changes size
    assert C.sizeof(pt.PtrSettings) == 144
    assert C.sizeof(pt.PtrSceneDesc) == 80
    assert C.sizeof(pt.PtrMaterial) == 576


def test_cli_accepts_metal_envlod_semantics():
    exe = pt.CLI_PATH
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "metal-envlod" in r.stdout
    for flags in (["--semantics=metal-envlod"], ["--semantics", "metal-envlod"], ["--backend=metal", "--semantics=metal-envlod"]):
        r = subprocess.run([exe, "--scene=/nonexistent.scene"] + flags, capture_output=True, text=True)
        assert r.returncode == 1 and "Failed to load scene" in r.stderr and "Invalid value" not in r.stderr, flags
    r = subprocess.run([exe, "--scene=x.scene", "--semantics=bogus"], capture_output=True, text=True)
    assert r.returncode == 1 and "Invalid value for --semantics" in r.stderr
