"""Rule 1 of the first-hit feature buffers (include/ptr_abi.h, ptr_render_aovs), stated in numpy on what the oracle reports: no code of
the kernels, and none of the package's.

Inputs are the host scene description (a PtrSceneDesc), the oracle's closest hits of the camera rays (PtrHit records: which primitive)
and its surface records of the same rays (OracleScene.surface_hits: geometric normal as stored, shading normal of the hit record, front
face).  first_hit_features runs the rule in the dtype asked for: float64 is the reference, float32 its twin, and the largest difference
between the two over a case is the unit of the tolerance of tests/test_gpu_aovs.py.
"""
import numpy as np

DIELECTRIC = 2
FACE_NORMAL = 4      # PTR_METAL_FACE_NORMAL
NORMAL_FLOOR = 2.0 ** -22   # two float32 ulps of an encoded normal near 1


def material_table(desc):
    """(base colour factors [m, 3] float32 clamped to [0, 1], types [m])"""
    m = int(desc.materialCount)
    base = np.array([list(desc.materials[i].baseColorRoughness)[:3] for i in range(m)], np.float32).reshape(m, 3)
    types = np.array([int(desc.materials[i].typeEta[0]) for i in range(m)], np.int64)
    return np.clip(base, np.float32(0.0), np.float32(1.0)), types


def hit_materials(desc, hits):
    """The material index the scene description gives the primitive each PtrHit names (misses: 0), clamped to the table."""
    spheres = np.array([desc.spheres[i].materialIndex[0] for i in range(desc.sphereCount)], np.int64)
    rects = np.array([desc.rects[i].materialTwoSided[0] for i in range(desc.rectCount)], np.int64)
    meshes = np.array([desc.meshes[i].materialIndex for i in range(desc.meshCount)], np.int64)
    kind = hits["primType"].astype(np.int64)
    prim = hits["primIndex"].astype(np.int64)
    geom = hits["geomIndex"].astype(np.int64)
    out = np.zeros(len(hits), np.int64)
    hit = hits["t"] >= 0
    for k, table, index in ((0, meshes, geom), (1, spheres, prim), (2, rects, prim)):
        use = hit & (kind == k)
        if use.any():
            out[use] = table[index[use]]
    return np.minimum(out, max(int(desc.materialCount) - 1, 0))


def shade_normal(dtype, geometric, shading, front, types, metal_semantics):
    """Points 2-4 of rule 1 for rows of (geometric normal, hit shading normal, front-face flag, material type): the encoded normal."""
    g = np.asarray(geometric, dtype)
    n = np.array(shading, dtype)
    zero = (n * n).sum(axis=1) <= 0
    n[zero] = g[zero]
    glass = np.asarray(types) == DIELECTRIC
    flipped = -g if (metal_semantics & FACE_NORMAL) else g
    n[glass] = np.where(np.asarray(front, bool)[glass, None], g[glass], flipped[glass])
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]).astype(dtype))
    n = (n / length[:, None]).astype(dtype)
    return (n * dtype(0.5) + dtype(0.5)).astype(dtype)


def first_hit_features(desc, hits, surface, metal_semantics=0, dtype=np.float64):
    """Per ray: {"hit" [n] bool, "albedo" [n, 3] float32, "normal" [n, 3] dtype (encoded), "distance" [n] float32, "material" [n]}.
    hits: the oracle's PtrHit records; surface: its [n, 16] surface records of the same rays."""
    n = len(hits)
    res = {"hit": np.zeros(n, bool), "albedo": np.zeros((n, 3), np.float32), "normal": np.full((n, 3), 0.5, dtype),
           "distance": np.zeros(n, np.float32), "material": np.zeros(n, np.int64)}
    if int(desc.materialCount) == 0 or n == 0:
        return res
    base, types = material_table(desc)
    hit = hits["t"] >= 0
    material = hit_materials(desc, hits)
    res["hit"] = hit
    res["material"] = material
    res["albedo"][hit] = base[material[hit]]
    res["distance"][hit] = hits["t"][hit]
    res["normal"][hit] = shade_normal(dtype, surface[hit, 5:8], surface[hit, 8:11], surface[hit, 11] > 0, types[material[hit]], metal_semantics)
    return res


def normal_tolerance(ref64, ref32):
    """max(8 x the largest difference of the float32 twin from the reference over the case, 2^-22)"""
    hit = ref64["hit"]
    worst = float(np.abs(ref32["normal"][hit].astype(np.float64) - ref64["normal"][hit]).max()) if hit.any() else 0.0
    return max(8.0 * worst, NORMAL_FLOOR)
