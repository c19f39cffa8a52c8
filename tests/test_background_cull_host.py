"""The primary-ray bounds cull on the host (csrc/host/background_cull.{h,cpp} through ptr_background_debug_cull; no GPU).

The rule hands renderPass a pixel rectangle outside which no camera ray of any sample can reach the scene.  Checked here:
  - the rectangle against an independent float64 projection written below (a 3x3 solve per box corner, not the rule's own formulas);
  - conservativeness with rays: the oracle's camera code (the one test_camera_rays_match_oracle holds the device's against) for 16 random
    (jitter, lens) draws per culled pixel, and a float64 copy of it for the four pixel corners (with the extreme lens offsets), against the
    scene's true bounds in a float64 slab test: not one ray of a culled pixel may reach the box;
  - the cases in which nothing may be culled.
"""
import importlib
import math
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import traversal_ref as tr
import traversal_scenes as ts

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------------------- float64 reference
def camera64(s):
    """buildCamera (csrc/host/hip_backend.cpp; the reference's BuildCamera) in float64."""
    aspect = s.width / s.height
    vfov = min(max(s.cameraVerticalFov, 1.0), 179.0)
    h = math.tan(math.radians(vfov) * 0.5)
    distance = max(s.cameraDistance, 0.1)
    cp, sp, cy, sy = math.cos(s.cameraPitch), math.sin(s.cameraPitch), math.cos(s.cameraYaw), math.sin(s.cameraYaw)
    look_at = np.array(list(s.cameraTarget), np.float64)
    origin = look_at + distance * np.array([cp * cy, sp, cp * sy])
    w = (origin - look_at) / np.linalg.norm(origin - look_at)
    u = np.cross([0.0, 1.0, 0.0], w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    focus = s.cameraFocusDistance if s.cameraFocusDistance > 0 else distance
    horizontal, vertical = focus * (2 * h * aspect) * u, focus * (2 * h) * v
    lower_left = origin - 0.5 * horizontal - 0.5 * vertical - focus * w
    lens = focus * math.tan(math.radians(max(s.cameraDefocusAngle, 0.0) * 0.5))
    return dict(origin=origin, lower_left=lower_left, horizontal=horizontal, vertical=vertical, u=u, v=v, w=w, lens=lens)


def projected_rect(cam, width, height, lo, hi):
    """Bounding rectangle, in pixel coordinates (x right, y down), of the box corners seen from the camera's origin: per corner P the
    (u, v, t) with lowerLeft + u horizontal + v vertical = origin + t (P - origin).  None when a corner is not in front."""
    pts = []
    for k in range(8):
        p = np.array([hi[a] if (k >> a) & 1 else lo[a] for a in range(3)], np.float64)
        if np.dot(p - cam["origin"], -cam["w"]) <= 0.0:
            return None
        m = np.stack([cam["horizontal"], cam["vertical"], -(p - cam["origin"])], axis=1)
        uu, vv, t = np.linalg.solve(m, cam["origin"] - cam["lower_left"])
        assert t > 0
        pts.append((uu * width, (1.0 - vv) * height))
    pts = np.array(pts)
    return pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()


def reference_culled_share(cam, width, height, lo, hi):
    """Share of the pixels the reference projection alone puts outside the scene: the rectangle of the box grown by the lens radius, widened
    by the lens radius on the focal plane and by two pixels a side (more than the rule's margin)."""
    r = cam["lens"]
    rect = projected_rect(cam, width, height, np.asarray(lo) - r, np.asarray(hi) + r)
    if rect is None:
        return 0.0
    mx = r / np.linalg.norm(cam["horizontal"]) * width + 2.0
    my = r / np.linalg.norm(cam["vertical"]) * height + 2.0
    x0, x1 = max(rect[0] - mx, 0.0), min(rect[1] + mx, width)
    y0, y1 = max(rect[2] - my, 0.0), min(rect[3] + my, height)
    return 1.0 - max(x1 - x0, 0.0) * max(y1 - y0, 0.0) / (width * height)


def true_bounds(desc):
    tri, _, sph = tr.world_primitives(desc)
    pts = np.concatenate([tri.reshape(-1, 3), sph[:, :3] - sph[:, 3:], sph[:, :3] + sph[:, 3:]])
    return pts.min(axis=0), pts.max(axis=0)


def rays_hit_box(org, d, lo, hi):
    """float64 slab test, t >= 0, of rays [n, 3] + [n, 3] against the box"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - org) / d, (hi - org) / d
    near, far = np.fmin(t1, t2), np.fmax(t1, t2)
    parallel_outside = (d == 0.0) & ((org < lo) | (org > hi))
    return (np.fmin.reduce(far, axis=1) >= np.maximum(np.fmax.reduce(near, axis=1), 0.0)) & ~parallel_outside.any(axis=1)


def corner_rays(cam, width, height, xy):
    """cameraRay at the four corners of each pixel, with no lens offset and (with a lens) the four extreme ones"""
    offsets = [np.zeros(3)]
    if cam["lens"] > 0:
        offsets += [cam["lens"] * sgn * cam[axis] for axis in ("u", "v") for sgn in (-1.0, 1.0)]
    orgs, dirs = [], []
    for jx in (0.0, 1.0):
        for jy in (0.0, 1.0):
            uu = (xy[:, 0] + jx) / width
            vv = 1.0 - (xy[:, 1] + jy) / height
            d0 = cam["lower_left"] + uu[:, None] * cam["horizontal"] + vv[:, None] * cam["vertical"] - cam["origin"]
            for off in offsets:
                orgs.append(np.broadcast_to(cam["origin"] + off, d0.shape))
                dirs.append(d0 - off)
    return np.concatenate(orgs), np.concatenate(dirs)


# ------------------------------------------------------------------------------------------------------------------------- scenes
SPHERES = ts.HEAD + "sphere center=-0.7,0,0 radius=0.5 material=0\nsphere center=0.8,0.3,0.2 radius=0.35 material=0\n"


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cull")
    (tmp / "spheres.scene").write_text(SPHERES)
    loaded = {"cornell": ts.scene_a(), "room": ts.scene_d(tmp), "spheres": ts.load(tmp / "spheres.scene")}
    return {k: (h, true_bounds(h.desc)) for k, h in loaded.items()}


W, H = 320, 180
CORNELL = dict(cameraTarget=(278.0, 278.0, 278.0), cameraDistance=1078.0, cameraYaw=-1.5708, cameraPitch=0.0, cameraVerticalFov=40.0)
# name -> (scene, camera overrides, the rule must cull)
CASES = {
    "on-axis": ("cornell", CORNELL, True),
    "oblique": ("cornell", dict(CORNELL, cameraYaw=-1.2, cameraPitch=0.35, cameraDistance=1400.0), True),
    "narrow": ("cornell", dict(CORNELL, cameraVerticalFov=20.0, cameraDistance=3000.0, cameraYaw=-1.3), True),
    "wide-120": ("cornell", dict(CORNELL, cameraVerticalFov=120.0, cameraPitch=0.2), True),
    # the camera stands beside the box at (700, 278, 278) and looks along (-0.6, 0, 0.8): near corners lie behind it
    "partly-behind": ("cornell", dict(CORNELL, cameraTarget=(400.0, 278.0, 678.0), cameraDistance=500.0, cameraYaw=-0.9273), False),
    "inside": ("cornell", dict(CORNELL, cameraDistance=100.0), False),
    # the 3000 x 3000 floor is kept out of the tree: the tree's own box is the blob and the light, +-40 wide
    "oversize": ("room", dict(cameraTarget=(0.0, 10.0, 0.0), cameraDistance=9000.0, cameraYaw=1.0, cameraPitch=1.0, cameraVerticalFov=40.0), True),
    "spheres": ("spheres", dict(), True),
}


def settings_of(host, camera, lens):
    s = host.settings_for(width=W, height=H, max_depth=4)
    for k, v in camera.items():
        if k == "cameraTarget":
            s.cameraTarget[:] = v
        else:
            setattr(s, k, v)
    s.cameraDefocusAngle = 2.0 if lens else 0.0
    s.cameraFocusDistance = 0.0
    return s


def test_signature_matches_the_header():
    text = open(os.path.join(ROOT, "include", "ptr_background.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    declared = {name: params.count(",") + 1 for name, params in re.findall(r"\b(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert set(declared) == set(pt.BACKGROUND_SYMBOLS)
    lib = pt.load_library()
    for name, count in declared.items():
        assert len(pt._BACKGROUND_SIGNATURES[name][1]) == count and hasattr(lib, name)


def test_benchmark_rectangle_against_the_projection():
    host = pt.HostScene.load(os.path.join(SCENES, "cornell_mesh.scene"), SCENES)
    s = host.settings_for(width=1920, height=1080, max_depth=8)
    got = pt.background_cull(s, desc=host.desc)
    lo, hi = true_bounds(host.desc)
    assert np.array_equal(lo, [0, 0, 0]) and np.array_equal(hi, [555, 555, 555])
    assert got["bounds_valid"] and np.all(got["lo"] <= lo) and np.all(got["hi"] >= hi) and np.all(got["hi"] - got["lo"] <= 555.1)
    px0, px1, py0, py1 = projected_rect(camera64(s), 1920, 1080, lo, hi)
    x0, x1, y0, y1 = got["rect"]
    print("projection x [%.2f, %.2f] y [%.2f, %.2f]; rule x [%d, %d) y [%d, %d)" % (px0, px1, py0, py1, x0, x1, y0, y1))
    assert got["culling"]
    # every edge at or outside the projected one, by at most 3 pixels
    assert 0.0 <= px0 - x0 <= 3.0 and 0.0 <= x1 - px1 <= 3.0 and 0.0 <= py0 - y0 <= 3.0 and 0.0 <= y1 - py1 <= 3.0
    assert got["traced"] == (x1 - x0) * (y1 - y0) and got["traced"] + got["background"] == 1920 * 1080
    share = got["background"] / (1920 * 1080)
    print("culled share %.4f" % share)
    assert share >= 0.47   # the analytic 0.486 less the margin


def test_partitions_split_the_same_pixels():
    host = pt.HostScene.load(os.path.join(SCENES, "cornell_mesh.scene"), SCENES)
    s = host.settings_for(width=320, height=180, max_depth=8)
    whole = pt.background_cull(s, desc=host.desc)
    parts = [pt.background_cull(s, desc=host.desc, part=p, parts=3) for p in range(3)]
    assert all(p["rect"] == whole["rect"] and p["culling"] for p in parts)
    assert sum(p["traced"] for p in parts) == whole["traced"] and sum(p["background"] for p in parts) == whole["background"] > 0


def test_no_culling_by_mode(monkeypatch):
    host = ts.scene_a()
    s = settings_of(host, CORNELL, False)
    assert pt.background_cull(s, desc=host.desc)["culling"]
    assert not pt.background_cull(s, desc=host.desc, count=True)["culling"]   # the counting build mirrors the reference's rays
    flat = s.copy()
    flat.maxDepth = 0
    assert not pt.background_cull(flat, desc=host.desc)["culling"]            # a frame of depth 0 adds nothing, not even the background
    monkeypatch.setenv("PTR_BACKGROUND_CULL", "0")
    off = pt.background_cull(s, desc=host.desc)
    assert not off["culling"] and off["background"] == 0 and off["traced"] == W * H


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("case", list(CASES))
def test_culled_pixels_cannot_reach_the_scene(scenes, case, lens):
    key, camera, must_cull = CASES[case]
    host, (lo, hi) = scenes[key]
    s = settings_of(host, camera, lens)
    got = pt.background_cull(s, desc=host.desc)
    cam = camera64(s)
    assert (cam["lens"] > 0) == lens
    assert got["bounds_valid"] and np.all(got["lo"] <= lo) and np.all(got["hi"] >= hi)
    if case == "oversize":
        assert pt.debug_scene_geometry(host.desc)["oversize"] == 2 and hi[0] - lo[0] == 3000.0
    if not must_cull:
        assert not got["culling"] and got["background"] == 0, case
        return
    want = reference_culled_share(cam, W, H, lo, hi)
    share = got["background"] / (W * H)
    print("%s: reference share %.3f, rule %.3f, rect %s" % (case, want, share, got["rect"]))
    assert want >= 0.10                    # the reference projection alone says the case culls
    assert got["culling"] and share >= 0.10
    x0, x1, y0, y1 = got["rect"]
    ys, xs = np.mgrid[0:H, 0:W]
    outside = ~((xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1))
    xy = np.stack([xs[outside], ys[outside]], axis=1)
    assert len(xy) == got["background"]
    if len(xy) >= 20000:
        xy = xy[np.random.default_rng(20000).choice(len(xy), 20000, replace=False)]
    org, d = corner_rays(cam, W, H, xy.astype(np.float64))
    assert not rays_hit_box(org, d, lo, hi).any()
    xys = np.concatenate([np.concatenate([xy, np.full((len(xy), 1), k)], axis=1) for k in range(16)]).astype(np.uint32)
    rays, _ = ol.camera_rays(s, xys)
    assert not rays_hit_box(rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64), lo, hi).any()
