"""The primary-ray bounds cull on the device: a plain frame with PTR_BACKGROUND_CULL at its default (on) is the frame with
PTR_BACKGROUND_CULL=0, bit for bit - k_background writes what the path pool would have written for the pixels it never sees.

Every culled case also says, through the host probe, that at least a fifth of its pixels took the new kernel, so nothing passes vacuously.
helmet_env.scene's own camera stands inside the box of its 1200 x 1200 ground, where the rule culls nothing: that frame is the
"camera inside the box" case, and the environment cases look at the scene from outside that box."""
import importlib
import os

import numpy as np
import pytest

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")

pytestmark = pytest.mark.gpu

SPP = 8
BG_SKY, BG_ENVIRONMENT = 0, 2   # PtrBackgroundMode (include/ptr_abi.h): the sky gradient, the environment map


class Scene:
    def __init__(self, path, assets=None):
        self.host = pt.HostScene.load(str(path), assets)
        self.dev = pt.DeviceScene(self.host.desc, 0, keepalive=self.host)


@pytest.fixture(scope="module")
def cornell():
    return Scene(os.path.join(SCENES, "cornell_mesh.scene"), SCENES)


@pytest.fixture(scope="module")
def helmet():
    return Scene(os.path.join(SCENES, "helmet_env.scene"), SCENES)


def both(monkeypatch, render):
    """render() with the cull on (the default) and off"""
    monkeypatch.delenv("PTR_BACKGROUND_CULL", raising=False)
    on = render()
    monkeypatch.setenv("PTR_BACKGROUND_CULL", "0")
    off = render()
    monkeypatch.delenv("PTR_BACKGROUND_CULL")
    return on, off


def culled_share(scene, s, part=0, parts=1):
    got = pt.background_cull(s, scene=scene.dev, part=part, parts=parts)
    again = pt.background_cull(s, desc=scene.host.desc, part=part, parts=parts)   # the uploaded scene holds the bounds of its description
    assert all(got[k] == again[k] for k in ("culling", "rect", "traced", "background"))
    return got["background"] / max(got["background"] + got["traced"], 1) if got["culling"] else 0.0


def check_equal(monkeypatch, scene, s, min_share=0.20):
    share = culled_share(scene, s)
    on, off = both(monkeypatch, lambda: scene.dev.render_image(s, SPP))
    assert on[1].samples == off[1].samples == s.width * s.height * SPP
    assert np.isfinite(off[0]).all() and off[0].mean() > 0.0
    assert np.array_equal(on[0], off[0])
    assert share >= min_share, share
    return on[0]


def test_cornell_mesh(monkeypatch, cornell):
    s = cornell.host.settings_for(width=320, height=180, max_depth=8)
    check_equal(monkeypatch, cornell, s)


def test_cornell_mesh_in_three_partitions(monkeypatch, cornell):
    s = cornell.host.settings_for(width=320, height=180, max_depth=8)
    whole, _ = cornell.dev.render_image(s, SPP)
    bands = []
    for part in range(3):
        assert culled_share(cornell, s, part, 3) >= 0.20
        on, off = both(monkeypatch, lambda: cornell.dev.render(s, SPP, part, 3))
        assert np.array_equal(on[0], off[0]), part
        assert on[1].samples == off[1].samples
        bands.append(on[0])
    assert np.array_equal(pt.assemble_bands(bands, 320, 180), whole)


def test_cornell_mesh_in_several_passes(monkeypatch, cornell):
    # 3 samples per pixel and pass: passes of 3, 3 and 2 samples, the running sum kept in the output buffer between them
    s = cornell.host.settings_for(width=320, height=180, max_depth=8)
    monkeypatch.setenv("PTR_MAX_ITEMS", str(320 * 180 * 3))
    split = check_equal(monkeypatch, cornell, s)
    monkeypatch.delenv("PTR_MAX_ITEMS")
    whole, _ = cornell.dev.render_image(s, SPP)
    # against one pass only the order of eight float additions differs: a few roundings of 6e-8 each
    assert np.allclose(split, whole, rtol=1e-5, atol=1e-6)


HELMET_OUTSIDE = dict(cameraDistance=2200.0, cameraPitch=0.7)   # above and outside the box of the ground


@pytest.mark.parametrize("metal", [0, 31], ids=["embree-semantics", "metal-31"])
def test_helmet_env(monkeypatch, helmet, metal):
    # environment background, MIS against environment sampling, level-0 lookups
    s = helmet.host.settings_for(width=192, height=108, metalSemantics=metal, **HELMET_OUTSIDE)
    assert s.backgroundMode == BG_ENVIRONMENT and helmet.host.desc.envWidth > 0
    image = check_equal(monkeypatch, helmet, s)
    assert image[0, 0].max() > 0.0   # a corner pixel: background only, and lit by the map


def test_camera_inside_the_box(monkeypatch, helmet, cornell):
    # nothing is culled, and the frame is still the same
    s = helmet.host.settings_for(width=192, height=108)
    got = pt.background_cull(s, scene=helmet.dev)
    assert not got["culling"] and got["background"] == 0
    check_equal(monkeypatch, helmet, s, min_share=0.0)
    inside = cornell.host.settings_for(width=160, height=90, max_depth=4, cameraDistance=260.0)   # at z = 18, in front of the mesh
    assert not pt.background_cull(inside, scene=cornell.dev)["culling"]
    check_equal(monkeypatch, cornell, inside, min_share=0.0)


def test_sky_and_thin_lens(monkeypatch, tmp_path):
    (tmp_path / "sky.scene").write_text(
        "camera target=0,0,0 distance=6 yaw=0.4 pitch=0.3 vfov=40\nrenderer maxDepth=4 seed=7\n"
        "material type=lambert albedo=0.7,0.6,0.5\nsphere center=0,0,0 radius=1 material=0\n")
    scene = Scene(tmp_path / "sky.scene")
    s = scene.host.settings_for(width=160, height=90, cameraDefocusAngle=3.0, cameraFocusDistance=6.0)
    assert s.backgroundMode == BG_SKY
    image = check_equal(monkeypatch, scene, s)
    assert image[0, 0].min() > 0.0   # the sky
    scene.dev.close()


def test_counting_render_traces_every_pixel(monkeypatch, cornell):
    s = cornell.host.settings_for(width=320, height=180, max_depth=8)
    got = pt.background_cull(s, scene=cornell.dev, count=True)
    assert not got["culling"] and got["background"] == 0 and got["traced"] == 320 * 180
    on, off = both(monkeypatch, lambda: cornell.dev.render_image(s, SPP, count=True))
    counters = lambda st: (st.primaryRays, st.extendRays, st.shadowRays, st.shadedHits, st.triangleHits, st.extendNodesVisited,
                           st.extendLeafPrimTests, st.nodesVisited, st.leafPrimTests, st.shadowEarlyExits, st.samples)
    print("counters", counters(on[1]))
    assert counters(on[1]) == counters(off[1]) and np.array_equal(on[0], off[0])
    assert on[1].primaryRays == 320 * 180 * SPP          # every camera ray went through the pool
    assert counters(on[1]) == PARENT_COUNTERS


# test_counting_render_traces_every_pixel's counters as the commit before the cull reports them (same scene, size, spp, seed)
PARENT_COUNTERS = (460800, 1241743, 357296, 875168, 174103, 24593775, 3454154, 31081376, 4419237, 14799, 460800)
