"""Scenes, environment maps and inputs of the light tests (test_lights_host.py on the CPU, test_gpu_lights.py on the device).

Everything is generated: scenes as `.scene` text (plus edits of the loaded rectangles where the text format cannot say it) and maps as PFM
files in the test's tmp_path.
"""
import importlib
import os

import numpy as np

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

LAMBERT_ALBEDO = (0.8, 0.3, 0.3)   # material 0 of materials.scene: the override material of the float64 comparisons


def _materials():
    """The material lines of tests/golden/materials.scene (one of every .scene type: indices 0..10), then two emitters (11, 12)."""
    lines = [l for l in open(os.path.join(GOLDEN, "materials.scene")) if l.startswith("material ")]
    assert len(lines) == 11
    return "".join(lines) + "material type=diffuse_light emit=10,8,6\nmaterial type=diffuse_light emit=3,4,5\n"


def _receivers(k, plate):
    """Spheres of every material on a floor, a ceiling above the lights (receivers behind a light that faces down), a strip in the plane of
    the first light (cosine exactly 0) and one a few ulps under it (the 1e-6 cosine floor), a wall that touches the first light at a right
    angle (the marginal case of quirk Q9), a plate 1e-3 under it, and a wall 1e4 away.  k scales the coordinates."""
    s = lambda *v: ",".join("%.9g" % (x * k) for x in v)
    out = "".join("sphere center=%s radius=%.9g material=%d\n" % (s(-3.6 + 0.8 * m, 0.4, 1.5 if m % 2 else -1.5), 0.4 * k, m) for m in range(10))
    out += "rectangle x=%s y=%s z=%s normal=1 material=10\n" % (s(-8, 8), s(0), s(-8, 8))
    out += "rectangle x=%s y=%s z=%s normal=-1 material=0\n" % (s(-8, 8), s(6), s(-8, 8))
    out += "rectangle x=%s y=%s z=%s normal=-1 material=0\n" % (s(1.5, 2.5), s(4), s(-1, 1))
    out += "rectangle x=%s y=%s z=%s normal=-1 material=10\n" % (s(1), s(2, 4), s(-1, 1))
    if plate:
        out += "rectangle x=%s y=%s z=%s normal=1 material=0\n" % (s(-0.25, 0.25), s(3.999), s(-0.25, 0.25))
    out += "rectangle x=%s y=%s z=%s normal=-1 material=0\n" % (s(2.6, 3.6), "%.9g" % (np.float32(3.999999) * np.float32(k)), s(-1, 1))
    out += "rectangle x=%s y=%s z=%s normal=-1 material=10\n" % (s(10000), s(0.5, 3.5), s(-3000, 3000))
    return out


RECEIVER_RECTS = 7   # rectangles of _receivers (one fewer without the plate): the lights follow

# (x range, y, z range, normal sign, two-sided, material) of lights in the plane y = const, and one upright light
_OVERHEAD = ((-1, 1), 4, (-1, 1), -1, 0, 11)
_LIGHTS = {
    1: [_OVERHEAD],
    2: [_OVERHEAD, "upright"],
    8: [_OVERHEAD, "upright",
        ((-1, 1), 5, (-1, 1), -1, 0, 12),                # behind the first light, seen only past its edges
        ((-3, -2.999), 3, (-2, 2), -1, 0, 11),           # a sliver, 1e-3 wide
        ((3, 4), 3.5, (2, 3), -1, 0, 12), ((3.5, 4.5), 3.5, (2.5, 3.5), -1, 1, 11),   # coplanar, overlapping: ties
        ((-5, -4), 2.5, (3, 4), 1, 1, 12),               # two-sided, facing up
        "zero"],                                         # zero area: parallel edges
}
_LIGHTS[9] = _LIGHTS[8] + [((5, 6), 3, (-4, -3), -1, 0, 11)]


def light_scene(tmp_path, lights, scale=1.0, plate=True):
    """A scene with `lights` (1, 2, 8 or 9) rectangle lights over the receivers; scale: 1 (unit) or e.g. 137.5 (Cornell-size coordinates).
    The lights are the last rectangles, in the order of _LIGHTS.  plate=False leaves out the plate 1e-3 under the first light, which hides a
    sixteenth of it from everything below."""
    base = RECEIVER_RECTS if plate else RECEIVER_RECTS - 1
    k = scale
    s = lambda *v: ",".join("%.9g" % (x * k) for x in v)
    text = ("camera target=0,%.9g,0 distance=%.9g yaw=0.4 pitch=0.3 vfov=40\nrenderer maxDepth=4 seed=1337\nbackground solid=0,0,0\n" % (2 * k, 14 * k)
            + _materials() + _receivers(k, plate))
    zero = None
    for i, l in enumerate(_LIGHTS[lights]):
        if l == "upright":   # two-sided, in the plane x = -6: receivers on either side see it
            text += "rectangle x=%s y=%s z=%s normal=1 twoSided=1 material=12\n" % (s(-6), s(1, 3), s(-1, 1))
        elif l == "zero":
            zero = base + i
            text += "rectangle x=%s y=%s z=%s normal=-1 material=11\n" % (s(6, 6.5), s(3), s(4, 4.5))
        else:
            x, y, z, n, two, m = l
            text += "rectangle x=%s y=%s z=%s normal=%d twoSided=%d material=%d\n" % (s(*x), s(y), s(*z), n, two, m)
    p = tmp_path / ("lights_%d_%g_%d.scene" % (lights, scale, plate))
    p.write_text(text)
    host = pt.HostScene.load(str(p), str(tmp_path))
    assert host.desc.rectCount == base + lights
    if zero is not None:   # edgeV = 2 edgeU: a light of zero area whose edges are parallel, not null
        r = host.desc.rects[zero]
        for c in range(3):
            r.edgeV[c] = 2.0 * r.edgeU[c]
    return host


def lambert():
    """The override material of the float64 comparisons: a Lambert surface of albedo LAMBERT_ALBEDO."""
    host = pt.HostScene.load(os.path.join(GOLDEN, "materials.scene"))
    m = pt.PtrMaterial()
    pt.C.memmove(pt.C.byref(m), pt.C.byref(host.desc.materials[0]), pt.C.sizeof(pt.PtrMaterial))
    assert int(m.typeEta[0]) == 0 and tuple(round(v, 6) for v in list(m.baseColorRoughness)[:3]) == LAMBERT_ALBEDO
    return m


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def receiver_rays(n, seed, scale=1.0):
    """Rays [m, 6] float32 {origin, direction} whose hits cover the receivers, and their class per ray: 'near' (anything in the room),
    'plane' (the strip in the first light's plane), 'graze' (the strip a few ulps under it), 'wall' (the wall that touches it), 'close' (the plate 1e-3 under it), 'far' (the wall
    1e4 away), 'back' (the floor from underneath, spheres from inside)."""
    rng = np.random.default_rng(seed)
    k = scale
    parts, names = [], []

    def add(name, o, d):
        parts.append(np.concatenate([o * k, _unit(d)], axis=1))
        names.extend([name] * len(o))

    o = rng.uniform((-7, 0.2, -7), (7, 5.8, 7), (n, 3))
    add("near", o, rng.normal(size=(n, 3)))
    m = max(n // 8, 16)
    add("near", rng.uniform((-1.5, 1, -1.5), (1.5, 3, 1.5), (m, 3)), rng.normal(size=(m, 3)) * (0.3, 1, 0.3) - (0, 3, 0))   # the floor under the light
    add("plane", rng.uniform((1.55, 3, -0.9), (2.45, 3.5, 0.9), (m, 3)), np.tile((0.0, 1.0, 0.0), (m, 1)))
    add("wall", rng.uniform((0.2, 2.05, -0.9), (0.9, 3.99, 0.9), (m, 3)), np.tile((1.0, 0.0, 0.0), (m, 1)))
    add("close", np.concatenate([rng.uniform(-0.2, 0.2, (m, 1)), np.full((m, 1), 3.9995), rng.uniform(-0.2, 0.2, (m, 1))], axis=1),
        rng.normal(size=(m, 3)) * (0.2, 0.0, 0.2) - (0, 1, 0))
    add("graze", rng.uniform((2.65, 3, -0.9), (3.55, 3.5, 0.9), (m, 3)), np.tile((0.0, 1.0, 0.0), (m, 1)))
    add("far", rng.uniform((9, 0.6, -2000), (50, 3.4, 2000), (m, 3)), np.tile((1.0, 0.0, 0.0), (m, 1)))
    add("back", rng.uniform((-7, -3, -7), (7, -0.5, 7), (m, 3)), rng.normal(size=(m, 3)) * (0.2, 0, 0.2) + (0, 1, 0))
    centres = np.array([(-3.6 + 0.8 * j, 0.4, 1.5 if j % 2 else -1.5) for j in range(10)])
    add("back", centres[rng.integers(0, 10, m)] + rng.uniform(-0.1, 0.1, (m, 3)), rng.normal(size=(m, 3)))
    return np.concatenate(parts).astype(np.float32), np.array(names)


def write_env(path, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    pt.write_image(str(path), rgb, "pfm")
    return str(path)


def env_scene(tmp_path, rgb, name):
    """A Lambert sphere under the environment map rgb [H, W, 3]; returns (host scene, RGBA [H, W, 4] as the scene holds it)."""
    env = write_env(tmp_path / (name + ".pfm"), rgb)
    p = tmp_path / (name + ".scene")
    p.write_text("camera target=0,0,0 distance=4 yaw=0.3 pitch=0.2 vfov=40\nrenderer maxDepth=3 seed=7\nbackground env=%s\n"
                 "material type=lambert albedo=0.7,0.7,0.7\nsphere center=0,0,0 radius=1 material=0\n" % env)
    host = pt.HostScene.load(str(p), str(tmp_path))
    h, w = host.desc.envHeight, host.desc.envWidth
    rgba = np.ctypeslib.as_array(host.desc.envRgba, shape=(h, w, 4)).copy()
    return host, rgba


ENV_SIZES = {"64x32": (64, 32), "33x17": (33, 17), "7x5": (7, 5), "16x3": (16, 3), "1x1": (1, 1)}


def env_map(kind, w, h, seed=3):
    """Map contents: 'noise' (positive, two decades), 'spot' (one texel at 500 over 0.01), 'black_top' (noise under a black top row),
    'flat' (every texel equal: all alias thresholds are exactly 1; with a black texel in each row: thresholds of exactly 0 too)."""
    rng = np.random.default_rng(seed)
    rgb = np.exp(rng.uniform(np.log(0.05), np.log(5.0), (h, w, 3))).astype(np.float32)
    if kind == "spot":
        rgb[:] = 0.01
        rgb[h // 3, (2 * w) // 3] = 500.0
    elif kind == "black_top":
        rgb[0] = 0.0
    elif kind == "flat":
        rgb[:] = 0.5
        if w > 1:
            rgb[:, w // 2] = 0.0
    elif kind != "noise":
        raise ValueError(kind)
    return rgb


def env_u(tables, n, seed):
    """Random triples, then the edges: 0, 0.99999994, 1, k/H and k/W exactly, one ulp either side of them and of alias thresholds."""
    rng = np.random.default_rng(seed)
    h, w = tables["cond_threshold"].shape
    u = [rng.random((n, 3), dtype=np.float32)]
    edge = [0.0, 0.99999994, 1.0, 0.5] + [k / h for k in range(h)][:12] + [k / w for k in range(w)][:12]
    thr = np.concatenate([tables["marg_threshold"][:4], tables["cond_threshold"].ravel()[:8]]).astype(np.float32)
    # (row + threshold) / H lands on the alias decision of that row; the same for the first columns of row 0
    edge += [float((np.float32(r) + thr[r]) / np.float32(h)) for r in range(min(4, h))]
    edge += [float((np.float32(c) + tables["cond_threshold"][0, c]) / np.float32(w)) for c in range(min(4, w))]
    e = np.array(edge, np.float32)
    e = np.unique(np.concatenate([e, np.nextafter(e, np.float32(2)), np.nextafter(e, np.float32(-1))]))
    grid = np.stack(np.meshgrid(e, e, indexing="ij"), axis=-1).reshape(-1, 2)
    u.append(np.concatenate([grid, rng.random((len(grid), 1), dtype=np.float32)], axis=1).astype(np.float32))
    u.append(np.stack([rng.random(len(e), dtype=np.float32), rng.random(len(e), dtype=np.float32), e], axis=1))
    return np.concatenate(u).astype(np.float32)


def env_directions(w, h, rotation, n, seed):
    """Random directions, +-y, the -x seam (atan2 = +-pi with z = +-0), non-unit vectors, and directions a fraction of a texel either side
    of texel borders of the rotated map."""
    rng = np.random.default_rng(seed)
    d = [_unit(rng.normal(size=(n, 3)))]
    d.append(np.array([(0, 1, 0), (0, -1, 0), (-1, 0, 0.0), (-1, 0, -0.0), (1, 0, 0.0), (1, 0, -0.0), (-1, 1e-3, 0.0), (-1, -1e-3, -0.0),
                       (0, 0, 1), (0, 0, -1), (1e-30, 1, 1e-30), (3, 4, 12), (1e-4, -2e-4, 1e-4), (250, 10, -40)], np.float64))
    # around the texel borders: u = (i + e) / W, v = (j + e) / H for small signed e, rotated back into the world
    m = max(n // 4, 64)
    e = rng.choice((-1e-2, -1e-3, 1e-3, 1e-2, 0.5), (m, 2))
    u = (rng.integers(0, w, m) + e[:, 0]) / w
    v = np.clip((rng.integers(0, h + 1, m) + e[:, 1]) / h, 0.0, 1.0)
    theta, phi = v * np.pi, u * 2 * np.pi - np.pi
    mx, my, mz = np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)
    c, s = np.cos(rotation), np.sin(rotation)
    d.append(np.stack([mx * c + mz * s, my, -mx * s + mz * c], axis=1))
    return np.concatenate(d).astype(np.float32)
