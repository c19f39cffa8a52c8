"""Scenes of the rebuild tests (test_rebuild_host.py on the CPU, test_gpu_rebuild.py on the device; include/ptr_rebuild.h), and the
reference tree of a scene at a pose: rebuild_ref on the arrays the probes return."""
import os

import numpy as np

import deform_scenes as dsc
import dynamic_ref as dr
import rebuild_ref as rr
import traversal_scenes as ts

pt = ts.pt
GOLDEN = ts.GOLDEN
KEYS = ["A", "C", "D", "textured", "F-triangle", "F-coincident", "strip", "E", "soup", "quads"]


def soup_scene(tmp):
    """Two meshes, each 1500 small triangles, one per cell of a jittered 12 x 12 x 11 grid with margins: no shared edge or vertex, no
    rectangle, so no two hits tie.  Object space spans +-0.6; the meshes sit at x = -2 and x = +2.  (test_gpu_dynamic.py's scene.)"""
    rng = np.random.default_rng(11)
    for name in ("soup_a", "soup_b"):
        cells = rng.permutation(12 * 12 * 11)[:1500]
        c = np.stack([cells % 12, (cells // 12) % 12, cells // 144], axis=1) * 0.1 + 0.05 - np.array([0.6, 0.6, 0.55])
        v = c[:, None, :] + rng.uniform(-0.035, 0.035, (1500, 3, 3))
        with open(tmp / (name + ".obj"), "w") as f:
            f.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in v.reshape(-1, 3))
            f.writelines("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3) for k in range(1500))
    p = tmp / "soup.scene"
    p.write_text("camera target=0,0,0 distance=7 yaw=1.5708 pitch=0.2 vfov=40\nrenderer maxDepth=4 seed=1337\nbackground\n"
                 "material type=lambert albedo=0.7,0.5,0.3\nmaterial type=metal albedo=0.8,0.8,0.9 fuzz=0.1\n"
                 "mesh path=soup_a.obj translate=-2,0,0 material=0\nmesh path=soup_b.obj translate=2,0,0 material=1\n")
    return ts.load(p, str(tmp))


QUADS = 12   # per side


def quads_scene(tmp):
    """QUADS x QUADS separate small quads (a fan of four triangles about the centre each) on a jittered grid in the plane y = 0."""
    rng = np.random.default_rng(5)
    verts, faces = [], []
    for q in range(QUADS * QUADS):
        c = np.array([q % QUADS - QUADS / 2 + 0.5, 0.0, q // QUADS - QUADS / 2 + 0.5]) * 0.5 + rng.uniform(-0.05, 0.05, 3) * np.array([1, 0.2, 1])
        b = len(verts)
        verts += [c, c + (-0.1, 0, -0.1), c + (0.1, 0.01, -0.1), c + (0.1, 0, 0.1), c + (-0.1, 0.01, 0.1)]
        faces += [(b, b + 1, b + 2), (b, b + 2, b + 3), (b, b + 3, b + 4), (b, b + 4, b + 1)]
    return dsc._scene(tmp, "quads", verts, faces)


def scrambled(host, seed=9):
    """New vertex data for the quads: every quad moved, whole, to the place of another one (a random permutation)."""
    pos, nrm, _, _ = dsc.mesh_data(host)
    assert len(pos) == QUADS * QUADS * 5
    centres = pos[0::5].astype(np.float64)
    perm = np.random.default_rng(seed).permutation(len(centres))
    step = np.repeat(centres[perm] - centres, 5, axis=0)
    return (pos + step).astype(np.float32), nrm


def host_scene(key, tmp):
    if key == "textured":
        return pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN)
    if key in ("A", "C"):
        return ts.scene_a() if key == "A" else ts.scene_c()
    if key == "D":
        return ts.scene_d(tmp)
    if key == "E":
        return ts.scene_e(tmp, count=20000)
    if key == "soup":
        return soup_scene(tmp)
    if key == "strip":
        return dsc.scene_strip(tmp, 257)
    if key == "quads":
        return quads_scene(tmp)
    return ts.scene_f(tmp, key[2:])


def padded_bounds(corners):
    """The padded bounds of triangles given as world-space corners [t, 3, 3] float32 (storeTri + padBounds of the host bake): [t, 2, 4]."""
    c = np.asarray(corners, np.float32)
    lo, hi = c.min(axis=1), c.max(axis=1)
    pad = np.float32(1e-5) * np.maximum(np.maximum(np.abs(lo), np.abs(hi)), np.float32(1.0))
    out = np.zeros((len(c), 2, 4), np.float32)
    out[:, 0, :3], out[:, 1, :3] = lo - pad, hi + pad
    return out


def reference_tree(nodes, tri_bounds, sphere_bounds):
    """What ptr_scene_rebuild_tree must build over the tree `nodes` (fitted to these bounds): (float nodes [n, 4, 4], schedule, level offsets)."""
    leaves = rr.leaf_table(nodes)
    lo, hi = dr.root_box(nodes)
    refs, _ = rr.rebuild(leaves, tri_bounds, sphere_bounds, lo, hi)
    return rr.fitted(refs, tri_bounds, sphere_bounds)
