"""Scenes and ray classes of the traversal tests (test_traversal_host.py on the CPU, test_gpu_traversal.py on the device).

Scenes written by a test go to its tmp_path as `.scene` text plus small OBJ / binary PLY files; the others are in the tree.
  A  tests/golden/cornell_small_mesh.scene (mesh, rectangles, a sphere)        B  tests/golden/materials.scene (sphere leaves)
  C  scenes/cornell_mesh.scene (70,688 triangles, the bench scene)            D  a room whose floor is kept out of the tree (oversize leaf)
  E  a hairball of thin random triangles whose rays reach the stack spill area  F  small and degenerate scenes
  G  scene A moved far from the origin, and scene A scaled down
"""
import importlib
import os

import numpy as np

import traversal_ref as tr

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(ROOT, "scenes")
EPS = np.float32(1e-4)

HEAD = ("camera target=0,0,0 distance=5 yaw=0.4 pitch=0.3 vfov=40\nrenderer maxDepth=4 seed=1337\nbackground solid=0.1,0.1,0.1\n"
        "material type=lambert albedo=0.6,0.6,0.6\nmaterial type=diffuse_light emit=10,10,10\n")

ROOM = ("camera target=0,10,0 distance=40 yaw=1.0 pitch=0.3 vfov=40\nrenderer maxDepth=5 seed=1337\nbackground solid=0.1,0.1,0.12\n"
        "material type=lambert albedo=0.6,0.6,0.6\nmaterial type=diffuse_light emit=14,14,14\nmaterial type=lambert albedo=0.8,0.5,0.3\n"
        "rectangle x=-1500,1500 y=0 z=-1500,1500 normal=1 material=0\n"
        "rectangle x=-40,40 y=90 z=-40,40 normal=-1 material=1\n"
        "mesh path=assets/blob_70688.obj translate=0,10,0 scale=0.05 material=2\n")


def load(path, assets=None):
    return pt.HostScene.load(str(path), assets)


def _write_obj(path, verts, faces):
    with open(path, "w") as f:
        f.writelines("v %.9g %.9g %.9g\n" % tuple(v) for v in verts)
        f.writelines("f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in faces)


def scene_a():
    return load(os.path.join(GOLDEN, "cornell_small_mesh.scene"), SCENES)


def scene_b():
    return load(os.path.join(GOLDEN, "materials.scene"))


def scene_c():
    return load(os.path.join(SCENES, "cornell_mesh.scene"), SCENES)


def scene_d(tmp_path):
    p = tmp_path / "room.scene"
    p.write_text(ROOM)
    return load(p, SCENES)


def scene_e(tmp_path, count=200_000, seed=7):
    """A deterministic hairball: `count` thin triangles (0.15 long, 0.0003 wide) at random places and directions in the unit cube.  Long thin
    triangles make boxes that overlap along most rays, so the four-wide walk pushes three siblings at many levels."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (count, 3)).astype(np.float32)
    a = rng.normal(size=(count, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(a, rng.normal(size=(count, 3)))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    v = np.stack([c, c + 0.15 * a, c + 0.0003 * b], axis=1).astype(np.float32).reshape(-1, 3)
    p = tmp_path / "hairball.ply"
    with open(p, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), count)).encode())
        f.write(v.astype("<f4").tobytes())
        faces = np.zeros(count, dtype=[("n", "u1"), ("i", "<i4", (3,))])
        faces["n"] = 3
        faces["i"] = np.arange(count * 3, dtype=np.int32).reshape(-1, 3)
        f.write(faces.tobytes())
    s = tmp_path / "hairball.scene"
    s.write_text(HEAD + "mesh path=hairball.ply material=0\n")
    return load(s, str(tmp_path))


def scene_f(tmp_path, which):
    """F: 'triangle' (the root reference is a leaf), 'sphere', 'coincident' (nine copies of one triangle: a full leaf plus one), 'flat'
    (every triangle in y = 0: one grid axis of zero extent), 'empty' (no primitive)."""
    body = ""
    if which == "triangle":
        _write_obj(tmp_path / "one.obj", [(-1, -0.5, 0.2), (1, -0.4, -0.1), (0.1, 1, 0)], [(0, 1, 2)])
        body = "mesh path=one.obj material=0\n"
    elif which == "sphere":
        body = "sphere center=0.1,0.2,-0.1 radius=0.8 material=0\n"
    elif which == "coincident":
        _write_obj(tmp_path / "nine.obj", [(-1, -0.5, 0.2), (1, -0.4, -0.1), (0.1, 1, 0)], [(0, 1, 2)] * 9)
        body = "mesh path=nine.obj material=0\n"
    elif which == "flat":
        rng = np.random.default_rng(5)
        verts, faces = [], []
        for k in range(200):   # one triangle per cell of a 20 x 10 grid: no two overlap (coplanar overlaps would all be ties)
            x, z = -2.0 + 0.2 * (k % 20), -2.0 + 0.4 * (k // 20)
            for dx, dz in ((0.0, 0.0), (rng.uniform(0.05, 0.18), rng.uniform(0.0, 0.1)), (rng.uniform(0.0, 0.18), rng.uniform(0.15, 0.38))):
                verts.append((x + dx, 0.0, z + dz))
            faces.append((3 * k, 3 * k + 1, 3 * k + 2))
        _write_obj(tmp_path / "flat.obj", verts, faces)
        body = "mesh path=flat.obj material=0\nrectangle x=-0.5,0.5 y=0 z=2.5,3.5 normal=1 material=1\n"
    elif which != "empty":
        raise ValueError(which)
    p = tmp_path / ("f_%s.scene" % which)
    p.write_text(HEAD + body)
    return load(p, str(tmp_path))


def scene_g(tmp_path, which):
    """G: scene A translated by (2e4, -1e4, 3e4) ('far') or scaled by 1e-2 ('small')."""
    off, k = ((2e4, -1e4, 3e4), 1.0) if which == "far" else ((0.0, 0.0, 0.0), 1e-2)
    out = []
    for line in open(os.path.join(GOLDEN, "cornell_small_mesh.scene")):
        words = line.split()
        if words and words[0] in ("rectangle", "sphere", "mesh"):
            fixed = []
            for w in words:
                key, _, val = w.partition("=")
                if key in ("x", "y", "z"):
                    a = "xyz".index(key)
                    val = ",".join("%.9g" % (float(t) * k + off[a]) for t in val.split(","))
                elif key in ("center", "translate"):
                    val = ",".join("%.9g" % (float(t) * k + off[a]) for a, t in enumerate(val.split(",")))
                elif key in ("radius", "scale"):
                    val = "%.9g" % (float(val) * k)
                fixed.append(key + "=" + val if val else w)
            line = " ".join(fixed) + "\n"
        elif words and words[0] == "camera":
            line = "camera target=%g,%g,%g distance=%g yaw=-1.5708 pitch=0 vfov=40\n" % (278 * k + off[0], 278 * k + off[1], 278 * k + off[2], 1078 * k)
        out.append(line)
    p = tmp_path / ("g_%s.scene" % which)
    p.write_text("".join(out))
    return load(p, SCENES)


# ------------------------------------------------------------------------------------------------------------------------------- rays
def bounds(ref):
    pts = np.concatenate([ref.tri.reshape(-1, 3), (ref.sph[:, :3] - ref.sph[:, 3:]), (ref.sph[:, :3] + ref.sph[:, 3:])])
    if len(pts) == 0:
        return np.array([-1.0, -1, -1]), np.array([1.0, 1, 1])
    return pts.min(axis=0), pts.max(axis=0)


def grid(ref):
    """gridOrigin, gridCell of the quantised nodes (csrc/host/bvh_builder.cpp: the root box = the padded primitive boxes, 65531 cells)."""
    lo, hi = [], []
    if len(ref.tri):
        t = ref.tri.astype(np.float32)
        lo.append(t.min(axis=1))
        hi.append(t.max(axis=1))
    if len(ref.sph):
        s = ref.sph.astype(np.float32)
        lo.append(s[:, :3] - s[:, 3:])
        hi.append(s[:, :3] + s[:, 3:])
    if not lo:   # (no primitive: the builder's unit cells)
        return np.zeros(3, np.float32), np.ones(3, np.float32)
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    pad = np.float32(1e-5) * np.maximum(np.maximum(np.abs(lo), np.abs(hi)), np.float32(1))
    lo, hi = (lo - pad).min(axis=0).astype(np.float64), (hi + pad).max(axis=0).astype(np.float64)
    ext = hi - lo
    cell = np.where(ext > 0, ext / 65531.0, 1.0)
    return (lo - 2.0 * cell).astype(np.float32), cell.astype(np.float32)


def pack(org, d, tmax=np.inf):
    org = np.asarray(org, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    tm = np.broadcast_to(np.asarray(tmax, np.float32), (org.shape[0],)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([org, np.full((org.shape[0], 1), EPS, np.float32), d, tm], axis=1), np.float32)


def _unit(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def random_rays(ref, n, seed):
    lo, hi = bounds(ref)
    c, r = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    rng = np.random.default_rng(seed)
    return pack(c + r * rng.uniform(-1.3, 1.3, (n, 3)), _unit(rng.normal(size=(n, 3))))


def aimed_rays(ref, n, seed, kinds=False):
    """Aimed at random points on primitives, at vertices and at edge midpoints (shared-edge ties), from random points around the scene.
    kinds: also return, per ray, whether it is aimed at a vertex or an edge midpoint (a tie by construction)."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(ref)
    c, r = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    targets = []
    if len(ref.tri):
        k = rng.integers(0, len(ref.tri), n)
        b = rng.dirichlet((1, 1, 1), n)
        kind = rng.integers(0, 3, n)
        b = np.where(kind[:, None] == 1, np.eye(3)[rng.integers(0, 3, n)], b)                    # vertices
        b = np.where(kind[:, None] == 2, (1 - np.eye(3)[rng.integers(0, 3, n)]) / 2, b)          # edge midpoints
        targets.append(np.einsum("rk,rkj->rj", b, ref.tri[k]))
    if len(ref.sph):
        k = rng.integers(0, len(ref.sph), n)
        targets.append(ref.sph[k, :3] + ref.sph[k, 3:] * _unit(rng.normal(size=(n, 3))))
    if not targets:
        rays = random_rays(ref, n, seed)
        return (rays, np.zeros(n, bool)) if kinds else rays
    edge = np.concatenate([kind != 0] + [np.zeros(len(x), bool) for x in targets[1:]]) if len(ref.tri) else np.zeros(len(targets[0]), bool)
    pick = rng.permutation(sum(len(x) for x in targets))[:n]
    t = np.concatenate(targets)[pick]
    org = c + r * rng.uniform(-1.4, 1.4, (len(t), 3))
    rays = pack(org, _unit(t - org))
    return (rays, edge[pick]) if kinds else rays


def axis_rays(ref, n, seed):
    """The six +-axis directions, and directions with exactly one or two zero components, zeros of both signs."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(ref)
    c, r = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    zeros = rng.integers(1, 3, n)                         # one or two zero components
    for i in range(n):
        for a in rng.permutation(3)[:zeros[i]]:
            d[i, a] = np.float32(-0.0) if rng.random() < 0.5 else np.float32(0.0)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)      # (keeps the sign of a zero)
    six = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    six = np.where(six == 0, np.where(rng.random(six.shape) < 0.5, np.float32(-0.0), np.float32(0.0)), six)
    d[:6 * (n // 12)] = np.tile(six, (n // 12, 1))
    return pack(c + r * rng.uniform(-1.1, 1.1, (n, 3)), d.astype(np.float32))


def grid_plane_rays(ref, n, seed):
    """Origins with one or more coordinates exactly on planes of the quantisation grid: gridOrigin + k * gridCell."""
    rng = np.random.default_rng(seed)
    origin, cell = grid(ref)
    lo, hi = bounds(ref)
    c, r = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    org = (c + r * rng.uniform(-1.1, 1.1, (n, 3))).astype(np.float32)
    for a in range(3):
        on = rng.random(n) < 0.6
        k = rng.integers(0, 65536, n).astype(np.float32)
        org[on, a] = (origin[a] + k[on] * cell[a]).astype(np.float32)
    d = _unit(rng.normal(size=(n, 3)))
    d[: n // 3, rng.integers(0, 3)] = 0.0
    return pack(org, d)


def inside_rays(ref, n, seed, points):
    """Origins near the given points (inside spheres / closed meshes), random directions."""
    rng = np.random.default_rng(seed)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    org = pts[rng.integers(0, len(pts), n)] + rng.normal(scale=1e-3, size=(n, 3)) * np.maximum(np.abs(pts).max(), 1.0)
    return pack(org, _unit(rng.normal(size=(n, 3))))


def grazing_rays(n, seed, y=0.0):
    """Rays in the plane y = `y` (scene F 'flat'): origins in the plane, directions with a zero y component of either sign."""
    rng = np.random.default_rng(seed)
    org = np.stack([rng.uniform(-3, 3, n), np.full(n, y), rng.uniform(-3, 3, n)], axis=1)
    d = rng.normal(size=(n, 3))
    d[:, 1] = 0.0
    d = _unit(d)
    d[::2, 1] = np.float32(-0.0)
    return pack(org, d)


def mixed_rays(ref, n, seed, inside=None, ties=False):
    """Every general ray class on one scene: random, aimed, axis-parallel / signed zeros, grid planes (and inside points).  ties: also
    return the mask of the rays aimed at vertices and edge midpoints."""
    aimed, edge = aimed_rays(ref, n, seed + 1, kinds=True)
    parts = [random_rays(ref, n, seed), aimed, axis_rays(ref, n // 2, seed + 2), grid_plane_rays(ref, n // 2, seed + 3)]
    if inside is not None:
        parts.append(inside_rays(ref, n // 4, seed + 4, inside))
    rays = np.concatenate(parts)
    mask = np.zeros(len(rays), bool)
    mask[n:n + len(aimed)] = edge
    return (rays, mask) if ties else rays


def deep_rays(desc, ref, n, seed, levels=16):
    """Rays of a scene whose four-wide walk holds more than `levels` stack entries (ptr_debug_walk_stack_depths), and their depths."""
    cand = np.concatenate([random_rays(ref, n, seed), aimed_rays(ref, n, seed + 1)])
    depth = pt.walk_stack_depths(desc, cand)
    return cand, depth
