"""The numpy restatement of what include/ptr_deform_device.h computes: the vertex adjacency a scene uploaded with PTR_DYNAMIC_VERTEX_NORMALS
keeps, and the area-weighted vertex normals k_dyn_vertex_normals derives through it.  float32 throughout, one rounding per operation
(numpy fuses nothing), in the order the header states: this is the only other statement of that rule."""
import numpy as np

F = np.float32


def adjacency(indices, vertex_count):
    """(offsets [vertex_count + 1], entries [corners]) of an index array [t, 3]: vertex v owns entries[offsets[v]:offsets[v + 1]], one
    per corner that names it, in ascending triangle order (a triangle naming v twice is there twice); an entry is the triangle's number."""
    corners = np.asarray(indices, np.int64).reshape(-1)
    assert not len(corners) or (corners.min() >= 0 and corners.max() < vertex_count)
    order = np.argsort(corners, kind="stable")   # stable: corners of one vertex stay in array order, which is triangle order
    offsets = np.zeros(vertex_count + 1, np.uint32)
    offsets[1:] = np.cumsum(np.bincount(corners, minlength=vertex_count))
    return offsets, (order // 3).astype(np.uint32)


def normals(positions, indices):
    """[n, 3] float32: per vertex the sum of cross(p1 - p0, p2 - p0) over its adjacency entries, in their order, one float32 add per
    component and entry; then n = d > 0 ? s * (1 / sqrt(d)) : s with d = (s.x s.x + s.y s.y) + s.z s.z.  (0, 0, 0) for a vertex no
    triangle names.  Overflow gives the non-finite values the device gives."""
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    n = len(pos)
    offsets, entries = adjacency(idx, n)
    with np.errstate(all="ignore"):
        p0, p1, p2 = pos[idx[:, 0]], pos[idx[:, 1]], pos[idx[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        cross = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(F)
        s = np.zeros((n, 3), F)
        valence = (offsets[1:] - offsets[:-1]).astype(np.int64)
        for k in range(int(valence.max()) if n else 0):   # the k-th entry of every vertex that has one: in-order sums, vertices side by side
            v = np.flatnonzero(valence > k)
            s[v] = s[v] + cross[entries[offsets[v].astype(np.int64) + k]]
        d = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        inv = F(1.0) / np.sqrt(d)
        out = np.where((d > 0)[:, None], s * inv[:, None], s).astype(F)
    assert cross.dtype == F and s.dtype == F and d.dtype == F and inv.dtype == F
    return out
