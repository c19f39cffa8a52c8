"""The small meshes of the include/ptr_deform_device.h tests (test_deform_device_host.py on the CPU, test_gpu_deform_device.py on the
device), given as arrays rather than files so that every vertex and index reaches the description as written: an unreferenced vertex, a
triangle that names one vertex three times and a vertex count of 1 would not survive a mesh loader."""
import ctypes as C

import numpy as np

import deform_device_ref as ref
import deform_scenes as dsc
import traversal_scenes as ts

pt = ts.pt


class Remeshed(dsc.Changed):
    """A copy of a host scene's description whose mesh `mesh` is replaced by positions [n, 3] and indices [t, 3]; its normals are the
    reference's (zeros where those are not finite) unless given.  No texture coordinates, no tangents."""

    def __init__(self, host, positions, indices, normals=None, mesh=0):
        super().__init__(host)
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
        if normals is None:
            normals = ref.normals(pos, idx)
            normals[~np.isfinite(normals).all(axis=1)] = 0.0
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self._keep.append((pos, nrm, idx))
        m = self._meshes[mesh]
        m.positions, m.normals = pos.ctypes.data_as(C.POINTER(C.c_float)), nrm.ctypes.data_as(C.POINTER(C.c_float))
        m.indices = idx.ctypes.data_as(C.POINTER(C.c_uint32))
        m.vertexCount, m.indexCount = len(pos), idx.size
        m.uv0 = m.uv1 = m.tangents = None
        self.positions, self.normals, self.indices = pos, nrm, idx


def fan(spokes=70):
    """A hub of valence `spokes`: more corners at one vertex than a wave has lanes."""
    k = np.arange(spokes)
    a = 2.0 * np.pi * k / spokes
    rim = np.stack([(1.0 + 0.2 * np.sin(5 * a)) * np.cos(a), (1.0 + 0.1 * np.cos(3 * a)) * np.sin(a), 0.15 * np.sin(2 * a + 0.3)], axis=1)
    verts = np.concatenate([[[0.05, -0.02, 0.4]], rim])
    faces = [(0, 1 + i, 1 + (i + 1) % spokes) for i in range(spokes)]
    return verts, faces


def odd():
    """Vertex 5 is named by no triangle; triangle 2 names vertex 1 twice (degenerate), triangle 3 names vertex 3 three times."""
    verts = [(-1, -0.5, 0.2), (1, -0.4, -0.1), (0.1, 1, 0), (1.2, 1.1, 0.3), (-0.8, 0.9, -0.2), (7, 7, 7)]
    return verts, [(0, 1, 2), (2, 1, 3), (1, 1, 4), (3, 3, 3), (4, 0, 2)]


def cancel():
    """Vertices 0, 1, 2 carry one triangle in both windings: the two cross products are each other's negatives and the sum is +0 in every
    component, whatever the positions; vertices 3 and 4 make the mesh more than that."""
    verts = [(-1, -0.5, 0.2), (1, -0.4, -0.1), (0.1, 1, 0), (1.2, 1.1, 0.3), (0.3, 0.2, 1.0)]
    return verts, [(0, 1, 2), (0, 2, 1), (2, 1, 3), (3, 1, 4)]


def strip(vertices):
    """A strip over `vertices` vertices (vertices - 2 triangles); with one vertex a single triangle that names it three times."""
    if vertices == 1:
        return [(0.3, -0.2, 0.1)], [(0, 0, 0)]
    k = np.arange(vertices)
    verts = np.stack([0.02 * k - 2.5, np.where(k % 2 == 0, -0.3, 0.3) + 0.05 * np.sin(0.37 * k), 0.2 * np.cos(0.11 * k)], axis=1)
    return verts, [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(vertices - 2)]


MESHES = {"fan": fan, "odd": odd, "cancel": cancel, "strip1": lambda: strip(1), "strip255": lambda: strip(255), "strip256": lambda: strip(256),
          "strip257": lambda: strip(257)}


def remeshed(tmp, key):
    """The one-mesh scene of ts.scene_f(tmp, "triangle") with its mesh replaced by MESHES[key]."""
    verts, faces = MESHES[key]()
    return Remeshed(ts.scene_f(tmp, "triangle"), verts, faces)


def moved(positions, seed=5):
    """New positions for a mesh: every vertex displaced by up to a third of the mesh's box (float32, finite)."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    box = float(np.max(pos.max(axis=0) - pos.min(axis=0))) or 1.0
    return (pos + np.random.default_rng(seed).uniform(-1.0, 1.0, pos.shape) * box / 3.0).astype(np.float32)
