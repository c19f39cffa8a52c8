"""Descriptions and scenes of the deformation tests (test_dynamic_deform_host.py on the CPU, test_gpu_dynamic_deform.py on the device):
a copy of a host scene's description with new vertex data, matrices, spheres and rectangles, which is what a fresh upload is given where
the device scene was updated; and the small meshes those tests deform."""
import ctypes as C

import numpy as np

import traversal_scenes as ts

pt = ts.pt


def mesh_data(host, mesh=0):
    """positions [n, 3], normals [n, 3], tangents [n, 4] or None, indices [t, 3] of mesh `mesh` of the description, copied."""
    m = host.desc.meshes[mesh]
    n = m.vertexCount
    pos = np.ctypeslib.as_array(m.positions, (n, 3)).copy()
    nrm = np.ctypeslib.as_array(m.normals, (n, 3)).copy()
    tan = np.ctypeslib.as_array(m.tangents, (n, 4)).copy() if m.tangents else None
    idx = np.ctypeslib.as_array(m.indices, (m.indexCount // 3, 3)).copy()
    return pos, nrm, tan, idx


class Changed:
    """A copy of a host scene's description with other vertex data ({mesh: (positions, normals[, tangents])}), matrices ({mesh: 4x4,
    row / column}), spheres ({index: (cx, cy, cz, r)}) and rectangles ({index: PtrRectUpdate}); everything else is the host's."""

    def __init__(self, host, vertices=None, matrices=None, spheres=None, rects=None):
        self._host = host
        d = host.desc
        self._keep = []
        self.desc = pt.PtrSceneDesc()
        C.memmove(C.byref(self.desc), C.byref(d), C.sizeof(pt.PtrSceneDesc))
        self._meshes = (pt.PtrMeshDesc * max(d.meshCount, 1))()
        for i in range(d.meshCount):
            C.memmove(C.byref(self._meshes[i]), C.byref(d.meshes[i]), C.sizeof(pt.PtrMeshDesc))
        fp = C.POINTER(C.c_float)
        for i, data in (vertices or {}).items():
            arrays = [np.ascontiguousarray(a, np.float32) for a in data]
            self._keep.append(arrays)
            self._meshes[i].positions, self._meshes[i].normals = arrays[0].ctypes.data_as(fp), arrays[1].ctypes.data_as(fp)
            if len(arrays) > 2:
                self._meshes[i].tangents = arrays[2].ctypes.data_as(fp)
        for i, m in (matrices or {}).items():
            self._meshes[i].localToWorld[:] = np.asarray(m, np.float32).T.reshape(-1).tolist()
        self.desc.meshes = C.cast(self._meshes, C.POINTER(pt.PtrMeshDesc))
        self._spheres = (pt.PtrSphere * max(d.sphereCount, 1))()
        for i in range(d.sphereCount):
            C.memmove(C.byref(self._spheres[i]), C.byref(d.spheres[i]), C.sizeof(pt.PtrSphere))
        for i, row in (spheres or {}).items():
            self._spheres[i].centerRadius[:] = np.asarray(row, np.float32).tolist()
        self.desc.spheres = C.cast(self._spheres, C.POINTER(pt.PtrSphere))
        self._rects = (pt.PtrRect * max(d.rectCount, 1))()
        for i in range(d.rectCount):
            C.memmove(C.byref(self._rects[i]), C.byref(d.rects[i]), C.sizeof(pt.PtrRect))
        for i, u in (rects or {}).items():
            for name in ("corner", "edgeU", "edgeV", "normalAndPlane"):
                getattr(self._rects[i], name)[:] = list(getattr(u, name))
        self.desc.rects = C.cast(self._rects, C.POINTER(pt.PtrRect))

    def settings_for(self, **kw):
        return self._host.settings_for(**kw)


def rect_of(host, index):
    """corner, edgeU, edgeV, normal (three components each) of rectangle `index` of the description."""
    r = host.desc.rects[index]
    return {"corner": np.array(list(r.corner)[:3], np.float32), "edgeU": np.array(list(r.edgeU)[:3], np.float32),
            "edgeV": np.array(list(r.edgeV)[:3], np.float32), "normal": np.array(list(r.normalAndPlane)[:3], np.float32)}


def _scene(tmp, name, verts, faces, extra=""):
    ts._write_obj(tmp / (name + ".obj"), verts, faces)
    p = tmp / (name + ".scene")
    p.write_text(ts.HEAD + "mesh path=%s.obj material=0\n" % name + extra)
    return ts.load(p, str(tmp))


def scene_pair(tmp):
    """Two triangles that share an edge: the gathered vertices 1 and 2 are read by both."""
    return _scene(tmp, "pair", [(-1, -0.5, 0.2), (1, -0.4, -0.1), (0.1, 1, 0), (1.2, 1.1, 0.3)], [(0, 1, 2), (2, 1, 3)])


def scene_strip(tmp, triangles=257):
    """A strip of `triangles` triangles over triangles + 2 vertices: with 257 it crosses a 256-thread block and leaves a one-lane tail."""
    k = np.arange(triangles + 2)
    verts = np.stack([0.02 * k - 2.5, np.where(k % 2 == 0, -0.3, 0.3) + 0.05 * np.sin(0.37 * k), 0.2 * np.cos(0.11 * k)], axis=1)
    faces = [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(triangles)]
    return _scene(tmp, "strip", verts, faces)


def displaced(host, mesh=0, seed=3, collapse=True):
    """New vertex data for a mesh: a per-vertex displacement that is a few scene boxes long for a third of the vertices, moderate for
    another third and zero for the rest; the first triangle collapsed to a point and the last vertex given the zero normal (collapse).
    Normals are turned, not recomputed: they are the caller's data, and any finite value must come through."""
    pos, nrm, tan, idx = mesh_data(host, mesh)
    rng = np.random.default_rng(seed)
    n = len(pos)
    box = float(np.max(pos.max(axis=0) - pos.min(axis=0))) if n else 1.0
    kind = np.arange(n) % 3
    step = rng.normal(size=(n, 3)) * np.where(kind == 0, 3.0 * box, np.where(kind == 1, 0.1 * box, 0.0))[:, None]
    pos2 = (pos + step).astype(np.float32)
    nrm2 = (nrm + rng.normal(size=(n, 3)) * 0.3).astype(np.float32)
    nrm2 /= np.maximum(np.linalg.norm(nrm2, axis=1, keepdims=True), 1e-20).astype(np.float32)
    if collapse and len(idx):
        pos2[idx[0]] = pos2[idx[0][0]]
        nrm2[n - 1] = 0.0
    out = [pos2, nrm2]
    if tan is not None:
        tan2 = tan.copy()
        tan2[:, :3] = (tan[:, :3] + rng.normal(size=(n, 3)) * 0.2).astype(np.float32)
        tan2[::5, 3] *= -1.0
        out.append(tan2)
    return tuple(out)


def original(host, mesh=0):
    pos, nrm, tan, _ = mesh_data(host, mesh)
    return (pos, nrm) if tan is None else (pos, nrm, tan)
