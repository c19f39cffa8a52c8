"""The per-hit material of the textured metallic-roughness model on classes of inputs: scenes built from numpy arrays, the input
classes, and a float64 statement of the rule.

The rule is the one stated in the header of csrc/kernels/texture.h (storage, mip chain, level of detail, filtering, the gradient
sample) and the reference shader's definition of the per-hit material (shaders/pathtrace.metal:108-198, 583-940, 2923-3216,
5919-6400).  `reference` states it in float64 from the scene as it is given to the C ABI - local positions, normals, tangents, uvs,
localToWorld, materials, texels - and takes from the side under test only the identity of the hit: mesh, triangle, bu, bv, t.  So it
also restates what the upload bakes: world positions, inverse-transpose normals, world tangents through the linear part with their
handedness times the sign of the determinant, uv-per-world with its area fallback.  Numbers of the rule that are float32 literals in
the shader are taken as the float32 value (T), so that an input equal to a threshold decides the same way.

For every decision of the rule the reference returns how far each row is from the threshold (`guards`).  A row nearer than GUARD[name]
is left out of the value comparison; its branch outcome is still recorded.  The classes are drawn so that no class leaves out more
than 2 % of its rows (tests/test_pbr_hit_host.py asserts it on the CPU).

Where the project's rule is its own and not the shader's it is said at the place: TANGENT_TRUST.
"""
import ctypes as C
import importlib

import numpy as np

pt = importlib.import_module("metal-pathtracer-arm64_amd")

NO_TEX = 0xFFFFFFFF
OWN = 0xFFFFFFFF
f32, f64 = np.float32, np.float64
ROWS = 4096
EPS32 = float(np.finfo(np.float32).eps)


def T(x):
    """A float32 literal of the rule as a float64 number."""
    return f64(f32(x))


# distance from a threshold below which a row is left out of the value comparison, per decision (units: see `reference`).  The 1e-4
# switch of the normal scale is decided per material on the float32 value itself (material/normal-scale has 1e-4 and 1.0001e-4): no row
# is near it.  The 1e-6 tests of the rule are on normalised vectors and only refuse a projection that vanishes ("projection").
GUARD = {
    "front": 1e-5,          # |cos| between the ray and the geometric normal (which side was hit)
    "hit_flip": 1e-5,       # |cos| between the interpolated normal and the geometric one (the surface record's flip)
    "mask": 1e-5,           # |alpha - cutoff|
    "blend": 1e-5,          # |draw - alpha|
    "nearest_texel": 1e-3,  # texels from a texel edge, NEAREST
    "nearest_level": 1e-3,  # levels from a rounding edge, NEAREST
    "tsign": 1e-5,          # ||tsign| - 0.5|
    "projection": 1e-12,    # squared length of a unit tangent's projection off the shading normal (refused where it vanishes)
    "len_1e-12": 1e-2,      # ... against 1e-12
    "denom_1e-8": 1e-2,     # ... of |denom| against 1e-8
    "handed": 1e-5,         # |(n x t) . bitangent| of the uv basis
    "nz": 1e-5,             # ||n.z| - 0.999|
    "map_flip": 1e-4,       # |mapped . ray-facing geometric normal|
    "aniso_ceil": 1e-3,     # distance of Pmax / Pmin from an integer below the tap limit
    "grad_window": 1e-2,    # relative distance of gradMag from 1e-6 and from 4
}


# --------------------------------------------------------------------------------------------- scenes
class Texture:
    def __init__(self, rgba, wrap_s=0, wrap_t=0, linear=True):
        self.rgba = np.ascontiguousarray(rgba, dtype=np.float32)
        self.wrap_s, self.wrap_t, self.linear = wrap_s, wrap_t, linear
        self._levels = None
        self._chain64 = None

    @property
    def levels(self):
        """The product's own float32 chain (ptr_debug_env_mips uses the material-texture chain rule)."""
        if self._levels is None:
            self._levels = pt.debug_env_mips(self.rgba)
        return self._levels

    @property
    def chain64(self):
        """The mip chain of the rule in float64: 2x2 box, odd sizes clamp the second tap, down to 1x1."""
        if self._chain64 is None:
            levels = [self.rgba.astype(f64)]
            while len(levels) < 16:
                s = levels[-1]
                h, w = s.shape[:2]
                if w == 1 and h == 1:
                    break
                nw, nh = max(w // 2, 1), max(h // 2, 1)
                x0, x1 = np.minimum(2 * np.arange(nw), w - 1), np.minimum(2 * np.arange(nw) + 1, w - 1)
                y0, y1 = np.minimum(2 * np.arange(nh), h - 1), np.minimum(2 * np.arange(nh) + 1, h - 1)
                levels.append((s[y0][:, x0] + s[y0][:, x1] + s[y1][:, x0] + s[y1][:, x1]) * 0.25)
            self._chain64 = levels
        return self._chain64


def pbr_material(base=(1.0, 1.0, 1.0), roughness=1.0, emission=(0.0, 0.0, 0.0), textures=None, uv_sets=None, transforms=None,
                 normal_scale=1.0, metallic=0.0, occlusion_strength=1.0, alpha=1.0, cutoff=0.5, transmission=0.0, alpha_mode=0.0,
                 two_sided=1.0, flags=0):
    """A metallic-roughness PtrMaterial; textures / uv_sets / transforms by slot: 0 base, 1 orm, 2 normal, 3 occlusion, 4 emissive,
    5 transmission.  alpha_mode: 0 OPAQUE, 1 MASK, 2 BLEND."""
    m = pt.PtrMaterial()
    m.baseColorRoughness[:] = [base[0], base[1], base[2], roughness]
    m.typeEta[:] = [7.0, 1.5, two_sided, 0.0]
    m.emission[:] = [emission[0], emission[1], emission[2], 0.0]
    m.carpaintBaseTint[:] = [1.0, 1.0, 1.0, 0.0]
    m.textureIndices0[:] = [NO_TEX] * 4
    m.textureIndices1[:] = [NO_TEX] * 4
    for slot, tex in (textures or {}).items():
        if slot < 4:
            m.textureIndices0[slot] = tex
        else:
            m.textureIndices1[slot - 4] = tex
    for slot, uv_set in (uv_sets or {}).items():
        if slot < 4:
            m.textureUvSet0[slot] = uv_set
        else:
            m.textureUvSet1[slot - 4] = uv_set
    for k in range(6):
        rows = (transforms or {}).get(k, ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
        m.textureTransform[2 * k][:] = [rows[0][0], rows[0][1], rows[0][2], 0.0]
        m.textureTransform[2 * k + 1][:] = [rows[1][0], rows[1][1], rows[1][2], 0.0]
    m.materialFlags = flags
    m.pbrParams[:] = [metallic, roughness, occlusion_strength, normal_scale]
    m.pbrExtras[:] = [alpha, cutoff, transmission, alpha_mode]
    return m


class Scene:
    """A PtrSceneDesc of triangle meshes and textures.  A mesh is a dict: positions [n, 3], indices [m, 3], material, and optionally
    uv0 [n, 2], uv1 [n, 2] (default: uv0), normals [n, 3] (default: +y), tangents [n, 4] (default: none) and l2w [4, 4] (the
    matrix that takes a local column vector to world space; default: identity).  "no_uv1": the mesh has no second set."""

    def __init__(self, meshes, materials, textures):
        self._keep = []
        keep = self._keep.append
        self.textures = textures
        self.meshes = meshes
        self.materials = materials
        self._dev = None
        self._bakes = {}
        desc = pt.PtrSceneDesc()
        mats = (pt.PtrMaterial * len(materials))(*materials)
        keep(mats)
        descs = (pt.PtrMeshDesc * len(meshes))()
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        for i, mesh in enumerate(meshes):
            pos = np.ascontiguousarray(mesh["positions"], dtype=np.float32)
            idx = np.ascontiguousarray(mesh["indices"], dtype=np.uint32)
            nrm = np.ascontiguousarray(mesh["normals"] if "normals" in mesh else np.broadcast_to(np.array([0.0, 1.0, 0.0], np.float32), pos.shape),
                                       dtype=np.float32)
            uv0 = np.ascontiguousarray(mesh["uv0"], dtype=np.float32) if mesh.get("uv0") is not None else None
            uv1 = None if mesh.get("no_uv1") else (np.ascontiguousarray(mesh["uv1"], dtype=np.float32) if mesh.get("uv1") is not None else uv0)
            tan = np.ascontiguousarray(mesh["tangents"], dtype=np.float32) if mesh.get("tangents") is not None else None
            l2w = np.ascontiguousarray(mesh.get("l2w", np.eye(4)), dtype=np.float32)
            mesh["_f32"] = {"positions": pos, "indices": idx.reshape(-1, 3), "normals": nrm, "uv0": uv0, "uv1": uv1, "tangents": tan, "l2w": l2w}
            keep((pos, idx, nrm, uv0, uv1, tan))
            d = descs[i]
            d.positions = pos.ctypes.data_as(fp)
            d.normals = nrm.ctypes.data_as(fp)
            d.indices = idx.ctypes.data_as(up)
            d.vertexCount, d.indexCount = pos.shape[0], idx.size
            d.localToWorld[:] = [float(x) for x in l2w.T.reshape(-1)]   # column-major
            d.materialIndex = mesh["material"]
            if uv0 is not None:
                d.uv0 = uv0.ctypes.data_as(fp)
            if uv1 is not None:
                d.uv1 = uv1.ctypes.data_as(fp)
            if tan is not None:
                d.tangents = tan.ctypes.data_as(fp)
        keep(descs)
        texs = (pt.PtrTexture * max(len(textures), 1))()
        for i, t in enumerate(textures):
            texs[i].rgba = t.rgba.ctypes.data_as(fp)
            texs[i].width, texs[i].height = t.rgba.shape[1], t.rgba.shape[0]
            texs[i].wrapS, texs[i].wrapT, texs[i].filter = t.wrap_s, t.wrap_t, 1 if t.linear else 0
        keep(texs)
        desc.materials, desc.materialCount = mats, len(materials)
        desc.meshes, desc.meshCount = descs, len(meshes)
        desc.textures, desc.textureCount = texs, len(textures)
        self.desc = desc

    @property
    def dev(self):
        if self._dev is None:
            self._dev = pt.DeviceScene(self.desc, 0, keepalive=self)
        return self._dev

    def bake64(self, mi):
        """What the upload bakes of mesh mi, in float64 from the float32 inputs."""
        if mi not in self._bakes:
            m = self.meshes[mi]["_f32"]
            M = m["l2w"].astype(f64)
            L = M[:3, :3]
            P = m["positions"].astype(f64) @ L.T + M[:3, 3]
            Nw = m["normals"].astype(f64) @ np.linalg.inv(L)        # (L^-1)^T n as row vectors
            ln = np.linalg.norm(Nw, axis=1, keepdims=True)
            Nw = np.where(ln > 0.0, Nw / np.where(ln > 0.0, ln, 1.0), Nw)
            det_sign = -1.0 if np.linalg.det(L) < 0.0 else 1.0
            nv = P.shape[0]
            if m["tangents"] is not None:
                tl = m["tangents"].astype(f64)
                Tw = tl[:, :3] @ L.T
                Ts = np.where(tl[:, 3] == 0.0, 0.0, np.where(tl[:, 3] < 0.0, -1.0, 1.0) * det_sign)
            else:
                Tw, Ts = np.zeros((nv, 3)), np.zeros(nv)
            uv0 = m["uv0"].astype(f64) if m["uv0"] is not None else np.zeros((nv, 2))
            uv1 = m["uv1"].astype(f64) if m["uv1"] is not None else np.zeros((nv, 2))
            self._bakes[mi] = {"P": P, "N": Nw, "T": Tw, "Ts": Ts, "det_sign": det_sign, "uv0": uv0, "uv1": uv1, "I": m["indices"].astype(np.int64)}
        return self._bakes[mi]


# --------------------------------------------------------------------------------------------- the rule in float64
def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rel(x, threshold):
    with np.errstate(invalid="ignore"):
        return np.abs(x / threshold - 1.0)


def rng_next(state):
    """The project's generator (csrc/kernels/bsdf.h rngNext): the state hashed, its low 24 bits as a fraction."""
    x = np.asarray(state, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32), (x & np.uint64(0x00FFFFFF)).astype(f64) / 16777216.0


def _wrap(i, n, mode):
    if mode == 1:
        return np.clip(i, 0, n - 1)
    if mode == 2:
        j = np.mod(i, 2 * n)
        return np.where(j < n, j, 2 * n - 1 - j)
    return np.mod(i, n)


def _filter_level(tex, level, u, v):
    """One level: bilinear with texel centres at (i + 0.5) / W, or for NEAREST the texel that holds (u, v) and how far that is from
    a texel edge."""
    img = tex.chain64[level]
    H, W = img.shape[:2]
    if not tex.linear:
        x, y = u * W, v * H
        edge = np.minimum(np.abs(x - np.round(x)), np.abs(y - np.round(y)))
        return img[_wrap(np.floor(y).astype(np.int64), H, tex.wrap_t), _wrap(np.floor(x).astype(np.int64), W, tex.wrap_s)], edge
    fx, fy = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[:, None], (fy - y0)[:, None]
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = _wrap(xi, W, tex.wrap_s), _wrap(xi + 1, W, tex.wrap_s)
    ya, yb = _wrap(yi, H, tex.wrap_t), _wrap(yi + 1, H, tex.wrap_t)
    return (img[ya, xa] * (1 - tx) + img[ya, xb] * tx) * (1 - ty) + (img[yb, xa] * (1 - tx) + img[yb, xb] * tx) * ty, np.full(len(u), np.inf)


def level_sample(tex, u, v, lod, guards):
    """The level sample: linear between the two nearest levels of bilinear lookups; NEAREST: one texel of the rounded level."""
    n = len(tex.chain64)
    l = np.clip(lod, 0.0, n - 1.0)
    out = np.zeros((len(u), 4))
    if not tex.linear:
        lv = np.floor(l + 0.5).astype(np.int64)
        guards["nearest_level"] = np.minimum(guards["nearest_level"], np.abs((l + 0.5) - np.round(l + 0.5)) if n > 1 else np.inf)
        for k in range(n):
            idx = lv == k
            if idx.any():
                out[idx], edge = _filter_level(tex, k, u[idx], v[idx])
                guards["nearest_texel"][idx] = np.minimum(guards["nearest_texel"][idx], edge)
        return out
    l0 = np.floor(l).astype(np.int64)
    frac = l - np.floor(l)
    for k in range(n):
        idx = l0 == k
        if not idx.any():
            continue
        a, _ = _filter_level(tex, k, u[idx], v[idx])
        if k + 1 < n:
            b, _ = _filter_level(tex, k + 1, u[idx], v[idx])
            a = a + (b - a) * frac[idx][:, None]
        out[idx] = a
    return out


def cone_lod(tex, uv_per_world, footprint):
    """ray_cone_lod_from_footprint: log2(footprint x uvPerWorld x max(W, H)), 0 where there is nothing to scale."""
    n = len(tex.chain64)
    H, W = tex.rgba.shape[:2]
    if n <= 1:
        return np.zeros(len(footprint))
    with np.errstate(divide="ignore", invalid="ignore"):
        lod = np.clip(np.log2(np.maximum(footprint * uv_per_world * max(W, H), T(1e-7))), 0.0, n - 1.0)
    return np.where((uv_per_world > 0.0) & (footprint > 0.0), lod, 0.0)


def _per_world(e1, e2, q0, q1, q2):
    """triangle_surface_partials' uv-per-world: from the partials, else from the areas, else 0."""
    d1, d2 = q1 - q0, q2 - q0
    det = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        dpdu = (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) / det[:, None]
        dpdv = (e2 * d1[:, 0:1] - e1 * d2[:, 0:1]) / det[:, None]
        lu, lv = np.linalg.norm(dpdu, axis=1), np.linalg.norm(dpdv, axis=1)
        per = np.maximum(1.0 / lu, 1.0 / lv)
        ok = (np.abs(det) > T(1e-9)) & (lu > T(1e-8)) & (lv > T(1e-8)) & np.isfinite(per) & (per > 0.0)
        world, uv = np.linalg.norm(np.cross(e1, e2), axis=1), np.abs(det)
        area = np.where((world > T(1e-12)) & (uv > T(1e-12)), np.sqrt(uv / world), 0.0)
    return np.where(ok, per, np.where(np.isfinite(area), area, 0.0))


def decode_normal(s, scale):
    """decode_normal_map: xy scaled, the length before z is rebuilt, z = sqrt(1 - xy^2), normalised."""
    n = s * 2.0 - 1.0
    n[:, 0] *= scale
    n[:, 1] *= scale
    length = np.linalg.norm(n, axis=1)
    n[:, 2] = np.sqrt(np.maximum(1.0 - (n[:, 0] ** 2 + n[:, 1] ** 2), 0.0))
    l2 = _dot(n, n)
    ok = l2 > T(1e-12)
    n = np.where(ok[:, None], n / np.sqrt(np.where(ok, l2, 1.0))[:, None], np.array([0.0, 0.0, 1.0]))
    return n, length


# The project's rule where it departs from the shader on purpose (DESIGN.md "per-hit material on classes of inputs"): a vertex tangent
# is trusted where the interpolated handedness has |w| > 0.5, so that w = 0 marks a vertex without a tangent.
TANGENT_TRUST = 0.5
FIELDS = ("base_color", "roughness", "emissive", "metallic", "transmission", "occlusion", "normal", "two_sided")


def reference(scene, rows, ident):
    """The per-hit material of rows [n, 20] (pt.DeviceScene.pbr_hit_rows) at the hits `ident` names (dict: hit, mesh, triangle, bu,
    bv, t).  Returns a dict: textured, discard, basis (the probe's code, + 4 flipped), state, front_face, geometric_normal,
    hit_normal, the FIELDS, lods, and guards: name -> distance of each row from that decision's threshold (inf: the decision was not
    taken)."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 20)
    words = rows.view(np.uint32)
    n = rows.shape[0]
    out = {"textured": np.zeros(n, bool), "discard": np.zeros(n, bool), "basis": np.zeros(n, np.uint32), "state": words[:, 8].copy(),
           "front_face": np.zeros(n, bool), "geometric_normal": np.zeros((n, 3)), "hit_normal": np.zeros((n, 3)),
           "base_color": np.zeros((n, 3)), "roughness": np.zeros(n), "emissive": np.zeros((n, 3)), "metallic": np.zeros(n),
           "transmission": np.zeros(n), "occlusion": np.zeros(n), "normal": np.zeros((n, 3)), "two_sided": np.zeros(n, bool),
           "lods": np.zeros((n, 2))}   # the level of detail the base-colour and the metallic-roughness lookups read at
    guards = {k: np.full(n, np.inf) for k in GUARD}
    out["guards"] = guards
    hit = np.asarray(ident["hit"]) > 0
    mesh_of = np.asarray(ident["mesh"]).astype(np.int64)
    wanted = words[:, 9].astype(np.int64)
    own = np.array([m["material"] for m in scene.meshes], dtype=np.int64)
    mat_of = np.minimum(np.where(wanted == OWN, own[np.clip(mesh_of, 0, len(own) - 1)], wanted), len(scene.materials) - 1)
    for mi in np.unique(mesh_of[hit]):
        for ma in np.unique(mat_of[hit & (mesh_of == mi)]):
            idx = np.nonzero(hit & (mesh_of == mi) & (mat_of == ma))[0]
            _reference_group(scene, int(mi), scene.materials[int(ma)], rows[idx], ident, idx, out)
    return out


def _reference_group(scene, mi, mat, rows, ident, idx, out):
    textures = scene.textures
    words = rows.view(np.uint32)
    k = len(idx)
    g = {name: np.full(k, np.inf) for name in GUARD}
    bk = scene.bake64(mi)
    I = bk["I"][np.asarray(ident["triangle"])[idx].astype(np.int64)]
    p0, p1, p2 = bk["P"][I[:, 0]], bk["P"][I[:, 1]], bk["P"][I[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    ng = _unit(np.cross(e1, e2))
    d = _unit(rows[:, 3:6].astype(f64))
    wo = -d
    cos_front = _dot(d, ng)
    front = cos_front < 0.0
    g["front"] = np.abs(cos_front)
    adjusted = np.where(front[:, None], ng, -ng)
    bu, bv = np.asarray(ident["bu"])[idx].astype(f64), np.asarray(ident["bv"])[idx].astype(f64)
    t_hit = np.asarray(ident["t"])[idx].astype(f64)
    # the surface record's shading normal: the interpolated vertex normal on the side the ray came from
    n0, n1, n2 = bk["N"][I[:, 0]], bk["N"][I[:, 1]], bk["N"][I[:, 2]]
    interp = (1.0 - bu - bv)[:, None] * n0 + bu[:, None] * n1 + bv[:, None] * n2
    has = _dot(interp, interp) > 0.0
    smooth = np.where(has[:, None], _unit(np.where(has[:, None], interp, 1.0)), adjusted)
    cos_flip = _dot(smooth, adjusted)
    g["hit_flip"] = np.where(has, np.abs(cos_flip), np.inf)
    sn = np.where((has & (cos_flip < 0.0))[:, None], -smooth, smooth)
    out["front_face"][idx], out["geometric_normal"][idx], out["hit_normal"][idx] = front, ng, sn
    if not (int(mat.typeEta[0]) == 7 and len(textures) > 0):
        return
    out["textured"][idx] = True
    # saturated barycentric weights, both uv sets, their uv-per-world
    w = np.maximum(np.stack([1.0 - bu - bv, bu, bv], axis=1), 0.0)
    ws = w.sum(axis=1)
    w = np.where((ws > T(1e-8))[:, None], w / np.where(ws > 0.0, ws, 1.0)[:, None], np.array([1.0, 0.0, 0.0]))
    corner = {s: [bk["uv%d" % s][I[:, c]] for c in range(3)] for s in (0, 1)}
    uv = {s: w[:, 0:1] * corner[s][0] + w[:, 1:2] * corner[s][1] + w[:, 2:3] * corner[s][2] for s in (0, 1)}
    per = {s: _per_world(e1, e2, *corner[s]) for s in (0, 1)}
    cone = rows[:, 6:8].astype(f64)
    footprint = np.maximum(cone[:, 0] + cone[:, 1] * np.maximum(t_hit, 0.0), T(1e-7)) / np.maximum(np.abs(_dot(ng, wo)), T(1e-3))
    tex_index = [mat.textureIndices0[0], mat.textureIndices0[1], mat.textureIndices0[2], mat.textureIndices0[3], mat.textureIndices1[0],
                 mat.textureIndices1[1]]
    uv_set = [min(x, 1) for x in (mat.textureUvSet0[0], mat.textureUvSet0[1], mat.textureUvSet0[2], mat.textureUvSet0[3], mat.textureUvSet1[0],
                                   mat.textureUvSet1[1])]
    valid = lambda s: tex_index[s] != NO_TEX and tex_index[s] < len(textures)
    inst1 = words[:, 10] != 0
    grads_in = rows[:, 11:19].astype(f64)
    grad_bits = words[:, 19]

    def slot(s):
        r0, r1 = np.array(mat.textureTransform[2 * s][:3], f64), np.array(mat.textureTransform[2 * s + 1][:3], f64)
        linear = abs(r0[0]) + abs(r0[1]) + abs(r1[0]) + abs(r1[1])
        if not (np.isfinite(r0).all() and np.isfinite(r1).all() and linear > T(1e-8)):
            r0, r1 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
        q = uv[uv_set[s]]
        scale = max(max(np.hypot(r0[0], r1[0]), np.hypot(r0[1], r1[1])), T(1e-6))
        gi = grads_in[:, 4 * uv_set[s]:4 * uv_set[s] + 4]
        with np.errstate(invalid="ignore", over="ignore"):
            gr = np.stack([r0[0] * gi[:, 0] + r0[1] * gi[:, 1], r1[0] * gi[:, 0] + r1[1] * gi[:, 1],
                           r0[0] * gi[:, 2] + r0[1] * gi[:, 3], r1[0] * gi[:, 2] + r1[1] * gi[:, 3]], axis=1)   # dudx, dvdx, dudy, dvdy
        has_grad = inst1 & (((grad_bits >> uv_set[s]) & 1) != 0) & np.isfinite(gr).all(axis=1)
        gr = np.where(has_grad[:, None], gr, 0.0)
        return {"u": r0[0] * q[:, 0] + r0[1] * q[:, 1] + r0[2], "v": r1[0] * q[:, 0] + r1[1] * q[:, 1] + r1[2],
                "per": per[uv_set[s]] * scale, "grad": gr, "has_grad": has_grad}

    def lod_of(tex, sl):
        """material_texture_lod_with_fallback: from the gradients where the slot has them and they give one, else the cone's."""
        lod = cone_lod(tex, sl["per"], footprint)
        H, W = tex.rgba.shape[:2]
        gr = np.abs(sl["grad"])
        rho = np.maximum(np.maximum(gr[:, 0] * W, gr[:, 1] * H), np.maximum(gr[:, 2] * W, gr[:, 3] * H))
        use = sl["has_grad"] & (len(tex.chain64) > 1) & np.isfinite(rho) & (rho > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            glod = np.clip(np.log2(np.maximum(rho, T(1e-8))), 0.0, len(tex.chain64) - 1.0)
        return np.where(use, glod, lod)

    def level(s, sl, fallback, du=0.0, dv=0.0):
        if not valid(s):
            return np.broadcast_to(np.array(fallback, f64), (k, 4)).copy()
        tex = textures[tex_index[s]]
        return level_sample(tex, sl["u"] + du, sl["v"] + dv, lod_of(tex, sl), g)

    def filtered(s, sl, fallback):
        """sample_material_texture_filtered: the gradient sample where the slot has non-zero gradients, else the level sample."""
        res = level(s, sl, fallback)
        if not valid(s):
            return res
        tex = textures[tex_index[s]]
        gr = sl["grad"]
        aniso = sl["has_grad"] & (np.abs(gr).max(axis=1) > 0.0)
        if not aniso.any():
            return res
        a = np.nonzero(aniso)[0]
        H, W = tex.rgba.shape[:2]
        levels = len(tex.chain64)
        px = np.hypot(gr[a, 0] * W, gr[a, 1] * H)
        py = np.hypot(gr[a, 2] * W, gr[a, 3] * H)
        x_major = px >= py
        pmax, pmin = np.where(x_major, px, py), np.where(x_major, py, px)
        limit = 8.0 if (tex.linear and levels > 1) else 1.0
        ratio = pmax / np.maximum(pmin, T(1e-6))
        nt = np.maximum(np.minimum(np.ceil(ratio), limit), 1.0)
        if limit > 1.0:
            g["aniso_ceil"][a] = np.minimum(g["aniso_ceil"][a], np.where(ratio < limit, np.abs(ratio - np.round(ratio)), np.inf))
        with np.errstate(divide="ignore"):
            lod = np.clip(np.log2(pmax / nt), 0.0, levels - 1.0)
        gu, gv = np.where(x_major, gr[a, 0], gr[a, 2]), np.where(x_major, gr[a, 1], gr[a, 3])
        ga = {name: np.full(len(a), np.inf) for name in GUARD}
        if not tex.linear:
            res[a] = level_sample(tex, sl["u"][a], sl["v"][a], lod, ga)
        else:
            total = np.zeros((len(a), 4))
            for i in range(8):
                on = i < nt
                if not on.any():
                    break
                o = (i + 0.5) / nt[on] - 0.5
                total[on] += level_sample(tex, sl["u"][a][on] + o * gu[on], sl["v"][a][on] + o * gv[on], lod[on], ga)
            res[a] = total / nt[:, None]
        # the level sample these rows did not take left its NEAREST distances in g: replace them by the gradient sample's
        for name in ("nearest_texel", "nearest_level"):
            g[name][a] = ga[name]
        return res

    one = (1.0, 1.0, 1.0, 1.0)

    def lookup(fn, s, sl, fallback):
        """One lookup of the rule, with the NEAREST distances of this lookup alone merged into those of the earlier ones."""
        before = {name: g[name].copy() for name in ("nearest_texel", "nearest_level")}
        g["nearest_texel"][:] = np.inf
        g["nearest_level"][:] = np.inf
        res = fn(s, sl, fallback)
        for name in before:
            g[name] = np.minimum(g[name], before[name])
        return res

    s_base = slot(0)
    base_sample = lookup(filtered, 0, s_base, one)
    for s in (0, 1):
        if valid(s):
            out["lods"][idx, s] = lod_of(textures[tex_index[s]], s_base if s == 0 else slot(1))
    bcr = np.array(mat.baseColorRoughness[:], f64)
    base_color = bcr[:3] * base_sample[:, :3]
    metallic = np.full(k, np.clip(f64(mat.pbrParams[0]), 0.0, 1.0))
    roughness = np.full(k, np.clip(f64(mat.pbrParams[1]), 0.0, 1.0))
    disable_orm = (mat.materialFlags & 1) != 0
    if not disable_orm and valid(1):
        mr = lookup(level, 1, slot(1), one)   # metallic-roughness always takes the level sample
        metallic = np.clip(mr[:, 2] * metallic, 0.0, 1.0)
        roughness = np.clip(mr[:, 1] * roughness, 0.0, 1.0)
    transmission = np.full(k, np.clip(f64(mat.pbrExtras[2]), 0.0, 1.0))
    if valid(5):
        transmission = np.clip(transmission * lookup(filtered, 5, slot(5), one)[:, 0], 0.0, 1.0)
    transmission = transmission * (1.0 - metallic)
    alpha = np.clip(np.clip(f64(mat.pbrExtras[0]), 0.0, 1.0) * base_sample[:, 3], 0.0, 1.0)
    state = words[:, 8].copy()
    discard = np.zeros(k, bool)
    mode = f64(mat.pbrExtras[3])
    if mode > 0.5:
        if mode < 1.5:
            cutoff = np.clip(f64(mat.pbrExtras[1]), 0.0, 1.0)
            discard = alpha < cutoff
            g["mask"] = np.abs(alpha - cutoff)
        else:
            state, draw = rng_next(state)
            discard = draw > alpha
            g["blend"] = np.abs(draw - alpha)
    out["state"][idx] = state
    out["discard"][idx] = discard
    occlusion = np.ones(k)
    if not disable_orm and valid(3):
        occ = lookup(filtered, 3, slot(3), one)[:, 0]
        occlusion = 1.0 + (occ - 1.0) * np.clip(f64(mat.pbrParams[2]), 0.0, 1.0)
    emissive = np.broadcast_to(np.array(mat.emission[:3], f64), (k, 3)).copy()
    if valid(4):
        emissive = emissive * lookup(filtered, 4, slot(4), one)[:, :3]
    normal = sn.copy()
    basis = np.zeros(k, np.uint32)
    scale = f64(mat.pbrParams[3])
    if valid(2) and scale > T(1e-4):
        s_n = slot(2)
        flat = (0.5, 0.5, 1.0, 1.0)
        nts, n_len = decode_normal(lookup(filtered, 2, s_n, flat)[:, :3], scale)
        # the vertex tangent: interpolated in world space, Gram-Schmidt against the shading normal
        t0, t1, t2 = bk["T"][I[:, 0]], bk["T"][I[:, 1]], bk["T"][I[:, 2]]
        tw = w[:, 0:1] * t0 + w[:, 1:2] * t1 + w[:, 2:3] * t2
        tsign = w[:, 0] * bk["Ts"][I[:, 0]] + w[:, 1] * bk["Ts"][I[:, 1]] + w[:, 2] * bk["Ts"][I[:, 2]]
        l2 = _dot(tw, tw)
        tw_ok = np.isfinite(tw).all(axis=1) & (l2 > T(1e-12))
        tw = np.where(tw_ok[:, None], tw / np.sqrt(np.where(tw_ok, l2, 1.0))[:, None], np.array([1.0, 0.0, 0.0]))
        trusted = np.abs(tsign) > TANGENT_TRUST
        g["tsign"] = np.abs(np.abs(tsign) - TANGENT_TRUST)
        g["len_1e-12"] = np.where(trusted, _rel(l2, T(1e-12)), np.inf)
        tv, tv_ok = _project(tw, sn)
        bv_ = _unit(np.cross(sn, tv)) * np.where(tsign < 0.0, -1.0, 1.0)[:, None]
        vertex = trusted & tv_ok & np.isfinite(bv_).all(axis=1)
        # ... else the triangle's uv derivatives of the normal map's set, in world space
        q0, q1, q2 = corner[uv_set[2]]
        du1, dv1, du2, dv2 = q1[:, 0] - q0[:, 0], q1[:, 1] - q0[:, 1], q2[:, 0] - q0[:, 0], q2[:, 1] - q0[:, 1]
        denom = du1 * dv2 - dv1 * du2
        with np.errstate(divide="ignore", invalid="ignore"):
            tan_w = (e1 * dv2[:, None] - e2 * dv1[:, None]) / denom[:, None]
            bit_w = (e2 * du1[:, None] - e1 * du2[:, None]) / denom[:, None]
            tl, bl = _dot(tan_w, tan_w), _dot(bit_w, bit_w)
            uv_ok = (np.abs(denom) >= T(1e-8)) & np.isfinite(tan_w).all(axis=1) & (tl > T(1e-12)) & np.isfinite(bit_w).all(axis=1) & (bl > T(1e-12))
            tan_w, bit_w = tan_w / np.sqrt(tl)[:, None], bit_w / np.sqrt(bl)[:, None]
        tan_w, bit_w = np.where(uv_ok[:, None], tan_w, 0.0), np.where(uv_ok[:, None], bit_w, 0.0)
        tu, tu_ok = _project(tan_w, sn)
        handed_cos = _dot(np.cross(sn, tu), bit_w)
        bu_ = _unit(np.cross(sn, tu)) * (np.where(handed_cos < 0.0, -1.0, 1.0) * bk["det_sign"])[:, None]
        from_uv = ~vertex & uv_ok & tu_ok
        g["denom_1e-8"] = np.where(~vertex & (np.abs(denom) > 0.0), _rel(np.abs(denom), T(1e-8)), np.inf)
        g["handed"] = np.where(from_uv, np.abs(handed_cos), np.inf)
        # ... else an arbitrary frame around the shading normal
        onb = ~vertex & ~from_uv
        g["nz"] = np.where(onb, np.abs(np.abs(sn[:, 2]) - T(0.999)), np.inf)
        up = np.where((np.abs(sn[:, 2]) < T(0.999))[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
        to = _unit(np.cross(up, sn))
        bo = np.cross(sn, to)
        tb = np.where(vertex[:, None], tv, np.where(from_uv[:, None], tu, to))
        bb = np.where(vertex[:, None], bv_, np.where(from_uv[:, None], bu_, bo))
        basis = np.where(vertex, 1, np.where(from_uv, 2, 3)).astype(np.uint32)
        mapped = _unit(tb * nts[:, 0:1] + bb * nts[:, 1:2] + sn * nts[:, 2:3])
        # ... kept on the side of the geometric normal *as the hit record has it*: turned towards the ray (set_face_normal,
        # M:1183-1193; M:6353 tests rec.normal), so a back-face hit keeps the mapped normal on the viewer's side
        cos_map = _dot(mapped, adjusted)
        g["map_flip"] = np.abs(cos_map)
        flipped = cos_map < 0.0
        normal = np.where(flipped[:, None], -mapped, mapped)
        basis = basis | np.where(flipped, 4, 0).astype(np.uint32)
        # shortened normals widen the lobe; with gradients so does the map's variation over the footprint
        tok = np.maximum((1.0 - n_len) / np.maximum(n_len, T(1e-6)), 0.0)
        mag = np.abs(s_n["grad"]).max(axis=1)
        window = s_n["has_grad"] & (mag > T(1e-6)) & (mag < 4.0)
        g["grad_window"] = np.where(s_n["has_grad"] & (mag > 0.0), np.minimum(_rel(mag, T(1e-6)), _rel(mag, 4.0)), np.inf)
        if window.any():
            ndx, _ = decode_normal(lookup(lambda s, sl, fb: level(s, sl, fb, sl["grad"][:, 0], sl["grad"][:, 1]), 2, s_n, flat)[:, :3], scale)
            ndy, _ = decode_normal(lookup(lambda s, sl, fb: level(s, sl, fb, sl["grad"][:, 2], sl["grad"][:, 3]), 2, s_n, flat)[:, :3], scale)
            variance = np.maximum(np.maximum(1.0 - _dot(nts, ndx), 0.0), np.maximum(1.0 - _dot(nts, ndy), 0.0))
            tok = tok + np.where(window, 0.35 * variance, 0.0)
        roughness = np.clip(np.sqrt(roughness * roughness + tok), 0.0, 1.0)
        g["projection"] = np.where(trusted, _project_length2(tw, sn), np.where(uv_ok, _project_length2(tan_w, sn), np.inf))
    out["basis"][idx] = basis
    out["base_color"][idx], out["roughness"][idx], out["emissive"][idx] = base_color, roughness, emissive
    out["metallic"][idx], out["transmission"][idx], out["occlusion"][idx], out["normal"][idx] = metallic, transmission, occlusion, normal
    out["two_sided"][idx] = f64(mat.typeEta[2]) > 0.5
    for name in GUARD:
        out["guards"][name][idx] = g[name]


# How a tangent is taken against the shading normal.  The shader normalises the projection and tests the *normalised* vector against
# 1e-6, so only a projection that vanishes (or is not finite) is refused; the 1e-6 tests of the rule are therefore never near.
def _project(tangent, normal):
    p = tangent - normal * _dot(normal, tangent)[:, None]
    unit = _unit(p)
    ok = np.isfinite(unit).all(axis=1) & (_dot(unit, unit) > T(1e-6))
    return np.where(ok[:, None], unit, 0.0), ok


def _project_length2(tangent, normal):
    p = tangent - normal * _dot(normal, tangent)[:, None]
    return _dot(p, p)


def guarded(ref):
    """Rows nearer to some threshold than its guard."""
    bad = np.zeros(len(ref["discard"]), bool)
    for name, limit in GUARD.items():
        bad |= ref["guards"][name] < limit
    return bad


# --------------------------------------------------------------------------------------------- textures and materials of every scene
def _build_textures():
    rng = np.random.default_rng(20260)
    tex, name = [], {}

    def add(key, t):
        name[key] = len(tex)
        tex.append(t)

    def noise(w, h, lo=0.05, hi=1.0):
        return rng.uniform(lo, hi, size=(h, w, 4))

    def normals(w, h, spread, length=None):
        xy = rng.uniform(-spread, spread, size=(h, w, 2))
        n = np.concatenate([xy, np.sqrt(1.0 - (xy ** 2).sum(axis=2, keepdims=True))], axis=2)
        if length is not None:
            n = n * rng.uniform(length[0], length[1], size=(h, w, 1))
        return np.concatenate([0.5 + 0.5 * n, np.ones((h, w, 1))], axis=2)

    add("base16", Texture(noise(16, 16), 0, 0, True))
    add("orm33", Texture(noise(33, 7), 2, 0, True))
    add("normal16", Texture(normals(16, 16, 0.6), 0, 0, True))
    add("occ5", Texture(noise(5, 3), 1, 1, True))
    add("emissive2", Texture(noise(2, 2, 0.2, 3.0), 0, 0, True))          # texels above 1
    add("trans1", Texture(np.full((1, 1, 4), 0.7), 0, 0, True))           # a single level
    add("near33", Texture(noise(33, 7), 2, 1, False))
    add("near16", Texture(noise(16, 16), 0, 0, False))
    for ws in range(3):
        for wt in range(3):
            for linear in (True, False):
                add("wrap%d%d%d" % (ws, wt, linear), Texture(noise(5, 3), ws, wt, linear))
    add("n_half", Texture(np.array([[[0.5, 0.5, 0.5, 1.0]]]), 0, 0, True))
    add("n_zero", Texture(np.array([[[0.0, 0.0, 0.0, 1.0]]]), 0, 0, True))
    add("n_one", Texture(np.array([[[1.0, 1.0, 1.0, 1.0]]]), 0, 0, True))
    add("n_short", Texture(normals(16, 16, 0.5, (0.25, 1.0)), 0, 0, True))
    return tex, name


def _build_materials(tx):
    mats, name = [], {}

    def add(key, **kw):
        name[key] = len(mats)
        mats.append(pbr_material(**kw))

    every = {0: tx["base16"], 1: tx["orm33"], 2: tx["normal16"], 3: tx["occ5"], 4: tx["emissive2"], 5: tx["trans1"]}
    common = dict(base=(0.9, 0.8, 0.7), roughness=0.8, emission=(0.6, 0.5, 0.4), metallic=0.9, occlusion_strength=0.7, transmission=0.6)
    add("all", textures=every, **common)
    add("all_one_sided", textures=every, two_sided=0.0, **common)
    add("normal_only", textures={2: tx["normal16"]}, **common)
    add("normal_uv1", textures={2: tx["normal16"]}, uv_sets={2: 1}, **common)
    for s in range(6):
        add("slot%d" % s, textures={s: every[s]}, **common)
    for u in (1, 2, 7):
        add("uvset%d" % u, textures=every, uv_sets={s: u for s in range(6)}, **common)
    c, s = np.cos(0.7), np.sin(0.7)
    rot = ((1.4 * c, -0.6 * s, 0.15), (1.4 * s, 0.6 * c, -0.25))
    add("xf_rot", textures=every, transforms={k: rot for k in range(6)}, **common)
    add("xf_zero", textures=every, transforms={k: ((0.0, 0.0, 0.3), (0.0, 0.0, 0.4)) for k in range(6)}, **common)
    add("xf_nan", textures=every, transforms={k: ((1.0, float("nan"), 0.0), (0.0, 1.0, 0.0)) for k in range(6)}, **common)
    add("xf_inf", textures=every, transforms={k: ((2.0, 0.0, 0.0), (0.0, 2.0, float("inf"))) for k in range(6)}, **common)
    for ws in range(3):
        for wt in range(3):
            for linear in (True, False):
                add("wrap%d%d%d" % (ws, wt, linear), textures={0: tx["wrap%d%d%d" % (ws, wt, linear)]},
                    transforms={0: ((3.1, 0.4, -1.3), (-0.5, 2.7, -0.8))}, **common)   # uv well outside [0, 1] on both sides
    add("orm_shared", textures={1: tx["orm33"], 3: tx["orm33"]}, **common)
    add("orm_shared_off", textures={1: tx["orm33"], 3: tx["orm33"]}, flags=1, **common)
    add("tex_at_count", textures={k: -1 for k in range(6)}, **common)      # patched below: the texture count itself
    add("tex_past_count", textures={k: 1000000 for k in range(6)}, **common)
    add("factors_a", textures=every, base=(1.5, 0.5, 0.25), roughness=-0.2, metallic=1.5, alpha=2.0, occlusion_strength=3.0, emission=(2.0, 1.0, 0.5))
    add("factors_b", textures=every, roughness=1.7, metallic=0.5, transmission=1.0, occlusion_strength=-1.0, alpha=-0.5)
    for i, scale in enumerate((0.0, 1.0e-4, 1.0001e-4, 1.0, 2.0, -1.0)):
        add("nscale%d" % i, textures={2: tx["normal16"]}, normal_scale=scale, **common)
    for key in ("n_half", "n_zero", "n_one", "n_short"):
        add(key, textures={2: tx[key]}, **common)
        add(key + "_x2", textures={2: tx[key]}, normal_scale=2.0, **common)
    add("emissive_hot", textures={4: tx["emissive2"]}, base=(1, 1, 1), emission=(2.0, 1.0, 0.5))
    add("opaque", textures={0: tx["base16"]}, alpha_mode=0.0, **common)
    add("mask", textures={0: tx["base16"]}, alpha_mode=1.0, cutoff=0.5, **common)
    add("mask_factor", textures={0: tx["base16"]}, alpha_mode=1.0, cutoff=0.3, alpha=0.6, **common)
    add("blend", textures={0: tx["base16"]}, alpha_mode=2.0, **common)
    add("near33", textures={0: tx["near33"], 2: tx["normal16"]}, **common)
    add("near16", textures={0: tx["near16"], 3: tx["near33"]}, **common)
    add("lods", textures={0: tx["base16"], 1: tx["orm33"], 2: tx["normal16"], 3: tx["near33"], 4: tx["near16"]}, **common)
    add("lambert", base=(0.5, 0.5, 0.5))
    mats[name["lambert"]].typeEta[0] = 0.0
    return mats, name


TEXTURES, TEX = _build_textures()
MATERIALS, MAT = _build_materials(TEX)
for _k in range(4):
    MATERIALS[MAT["tex_at_count"]].textureIndices0[_k] = len(TEXTURES)
MATERIALS[MAT["tex_at_count"]].textureIndices1[0] = len(TEXTURES)
MATERIALS[MAT["tex_at_count"]].textureIndices1[1] = len(TEXTURES)


# --------------------------------------------------------------------------------------------- meshes and scenes
def _rotation(axis, angle):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _l2w(linear, at):
    M = np.eye(4)
    M[:3, :3] = linear
    M[:3, 3] = at
    return M


TILTED = _rotation((1.0, 2.0, 0.5), 0.9)


def patch(seed, material=0, tilt=0.4, tangent_w=None, linear=TILTED, at=(0.0, 0.0, 0.0), uv="affine", normals="smooth", parallel=None):
    """Four triangles around a centre vertex in the local plane z = 0 (normal +z).  tilt: how far the vertex normals lean; tangent_w:
    None (no tangent array), a number, or one per vertex; uv: "affine", "constant" or "collinear" (set 0; set 1 stays affine), or
    "absent" (the mesh has neither set);
    normals: "smooth", "zero"; parallel: angle between every vertex tangent and its normal."""
    rng = np.random.default_rng(seed)
    xy = np.array([[0.0, 0.0], [-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]]) + rng.uniform(-0.15, 0.15, size=(5, 2))
    pos = np.concatenate([xy, np.zeros((5, 1))], axis=1)
    lean = rng.uniform(-tilt, tilt, size=(5, 2))
    nrm = np.concatenate([lean, np.ones((5, 1))], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    if normals == "zero":
        nrm = np.zeros((5, 3))
    phi = rng.uniform(-0.5, 0.5, size=5)
    tan = np.stack([np.cos(phi), np.sin(phi), rng.uniform(-0.3, 0.3, size=5)], axis=1)
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    if parallel is not None:
        side = tan - nrm * np.sum(tan * nrm, axis=1, keepdims=True)
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        tan = nrm * np.cos(parallel) + side * np.sin(parallel)
    A = np.array([[0.31, -0.12], [0.09, 0.27]])
    B = np.array([[-0.21, 0.33], [0.4, 0.18]])
    uv0 = xy @ A.T + np.array([0.4, 0.55])
    if uv == "constant":
        uv0 = np.broadcast_to(np.array([0.3, 0.6]), (5, 2)).copy()
    elif uv == "collinear":
        u = np.float32(0.2 * xy[:, 0] + 0.1 * xy[:, 1] + 0.5).astype(f64)
        uv0 = np.stack([u, 0.5 * u], axis=1)
    mesh = {"positions": pos, "indices": np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]]), "normals": nrm, "uv0": uv0,
            "uv1": xy @ B.T + np.array([0.1, 0.2]), "material": material, "l2w": _l2w(linear, at)}
    if uv == "absent":
        mesh["uv0"], mesh["no_uv1"] = None, True
    if tangent_w is not None:
        mesh["tangents"] = np.concatenate([tan, np.broadcast_to(np.asarray(tangent_w, f64), (5,)).reshape(5, 1)], axis=1)
    return mesh


MIRRORED = _rotation((0.3, 1.0, -0.4), 1.1) @ np.diag([1.3, 0.7, 2.0]) @ np.diag([1.0, -1.0, 1.0])
SHEARED = _rotation((1.0, 0.2, 0.7), 0.5) @ np.array([[1.0, 0.6, 0.2], [0.0, 1.0, 0.5], [0.0, 0.0, 1.2]])
FLAT = np.eye(3)
DOWN = _rotation((1.0, 0.0, 0.0), np.pi)
_GRID = [(40.0 * i, 0.0, 0.0) for i in range(8)]
PARALLEL = (1.0e-4, 3.0e-4, 6.0e-4, 1.5e-3, 4.0e-3, 1.0e-2)   # tangent/parallel: the angle between vertex tangent and normal, one mesh each


def _scene_meshes(name):
    g, A = _GRID, MAT["all"]
    if name == "vertex":
        return [patch(1, A, tangent_w=1.0, at=g[0]), patch(2, A, tangent_w=-1.0, at=g[1])]
    if name == "none_mixed":     # a mesh with no tangent array beside one that has it, and two with no uv set of their own
        return [patch(3, A, at=g[0]), patch(4, A, tangent_w=1.0, at=g[1]), patch(5, A, uv="absent", at=g[2]),
                patch(6, A, uv="absent", tangent_w=-1.0, at=g[3])]
    if name == "none":           # no mesh of the scene has tangents
        return [patch(5, A, at=g[0]), patch(6, MAT["normal_uv1"], at=g[1])]
    if name == "untrusted":      # w = 0 everywhere; signs that differ within every triangle
        return [patch(7, A, tangent_w=0.0, at=g[0]), patch(8, A, tangent_w=[1.0, -1.0, 1.0, -1.0, 1.0], at=g[1]),
                patch(9, A, tangent_w=[-1.0, 1.0, 0.0, 1.0, -1.0], at=g[2])]
    if name == "parallel":
        return [patch(10 + i, A, tilt=0.3, tangent_w=(1.0 if i % 2 == 0 else -1.0), parallel=a, at=(8.0 * i, 0.0, 0.0)) for i, a in enumerate(PARALLEL)]   # (near the origin: the positions' own rounding stays small)
    if name == "degenerate_uv":
        return [patch(20, A, uv="constant", at=g[0]), patch(21, A, uv="collinear", at=g[1]),
                patch(22, A, uv="constant", tilt=0.02, linear=FLAT, at=g[2]), patch(23, A, uv="collinear", tilt=0.02, linear=DOWN, at=g[3]),
                patch(24, MAT["normal_uv1"], uv="constant", at=g[4])]   # the normal map on the set that is not degenerate
    if name == "mirrored":
        return [patch(30, A, tangent_w=1.0, linear=MIRRORED, at=g[0]), patch(31, A, tangent_w=-1.0, linear=MIRRORED, at=g[1]),
                patch(32, A, linear=MIRRORED, at=g[2]), patch(33, MAT["normal_uv1"], linear=MIRRORED, at=g[3])]
    if name == "sheared":
        return [patch(40, A, tangent_w=1.0, linear=SHEARED, at=g[0]), patch(41, A, tangent_w=-1.0, linear=SHEARED, at=g[1]),
                patch(42, A, linear=SHEARED, at=g[2])]
    if name == "normal_zero":
        return [patch(50, A, normals="zero", tangent_w=1.0, at=g[0]), patch(51, A, normals="zero", at=g[1]),
                patch(52, A, normals="zero", uv="constant", linear=FLAT, at=g[2])]
    if name == "footprint":      # one patch and one whose uv-per-world is 0
        return [patch(60, MAT["lods"], tangent_w=1.0), patch(61, MAT["lods"], uv="constant", at=(0.0, 0.0, -200.0))]
    raise KeyError(name)


_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = Scene(_scene_meshes(name), MATERIALS, TEXTURES)
    return _scenes[name]


# --------------------------------------------------------------------------------------------- rows
def aim(sc, rng, n, meshes, back=0.0, cos=(0.05, 1.0), dist=(0.5, 4.0), bary="inside", log_dist=False):
    """n rays at points of the triangles of `meshes`: from the front of the geometric normal (a fraction `back` from behind), the
    cosine to the normal in `cos` (half of them log-uniform when cos[0] < 0.05), from a distance in `dist`; directions of length 0.5 .. 2."""
    rays = np.zeros((n, 6))
    mesh = rng.choice(np.asarray(meshes), size=n)
    for mi in np.unique(mesh):
        idx = np.nonzero(mesh == mi)[0]
        k = len(idx)
        bk = sc.bake64(int(mi))
        I = bk["I"][rng.integers(0, len(bk["I"]), size=k)]
        if bary == "inside":
            b = 0.02 + 0.94 * rng.dirichlet((1.0, 1.0, 1.0), size=k)
        else:   # vertices, points of edges, and points a rounding error to either side of an edge
            kind = rng.integers(0, 3, size=k)
            s = rng.uniform(0.0, 1.0, size=k)
            b = np.zeros((k, 3))
            corner = rng.integers(0, 3, size=k)
            b[np.arange(k), corner] = np.where(kind == 0, 1.0, s)
            b[np.arange(k), (corner + 1) % 3] = np.where(kind == 0, 0.0, 1.0 - s)
            nudge = np.where(kind == 2, rng.choice([-3e-7, 3e-7], size=k), 0.0)
            b[np.arange(k), (corner + 2) % 3] += nudge
            b[np.arange(k), corner] -= nudge
        p0, p1, p2 = bk["P"][I[:, 0]], bk["P"][I[:, 1]], bk["P"][I[:, 2]]
        P = b[:, 0:1] * p0 + b[:, 1:2] * p1 + b[:, 2:3] * p2
        ng = _unit(np.cross(p1 - p0, p2 - p0))
        side = np.where(rng.uniform(size=k) < back, -1.0, 1.0)
        c = rng.uniform(max(cos[0], 0.05), cos[1], size=k)
        if cos[0] < 0.05:   # half of the rows log-uniform down to grazing
            c = np.where(rng.uniform(size=k) < 0.5, 10.0 ** rng.uniform(np.log10(cos[0]), np.log10(cos[1]), size=k), c)
        inplane = _unit(np.cross(ng, rng.normal(size=(k, 3))))
        away = ng * (side * c)[:, None] + inplane * np.sqrt(1.0 - c * c)[:, None]
        d = 10.0 ** rng.uniform(np.log10(dist[0]), np.log10(dist[1]), size=k) if log_dist else rng.uniform(dist[0], dist[1], size=k)
        rays[idx, 0:3] = P + away * d[:, None]
        rays[idx, 3:6] = -away * rng.uniform(0.5, 2.0, size=k)[:, None]
    return rays


def _rows(sc, rng, n, meshes, materials=None, cones=None, **kw):
    rays = aim(sc, rng, n, meshes, **kw)
    if cones is None:
        cones = np.stack([10.0 ** rng.uniform(-3.0, -0.5, size=n), 10.0 ** rng.uniform(-3.0, -0.5, size=n)], axis=1)
    states = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    mats = None if materials is None else rng.choice(np.array([MAT[m] for m in materials], dtype=np.uint32), size=n)
    return pt.DeviceScene.pbr_hit_rows(rays, cones, states, mats)


def _geometry(scene_name, meshes, materials=None, **kw):
    return scene_name, lambda sc, rng: _rows(sc, rng, ROWS, meshes, materials, **kw)


def _material(materials, **kw):
    return "vertex", lambda sc, rng: _rows(sc, rng, ROWS, (0, 1), materials, **kw)


def _footprint(sc, rng):
    n = ROWS
    pick = lambda: np.where(rng.uniform(size=n) < 0.15, 0.0, 10.0 ** rng.uniform(-9.0, 1.0, size=n))
    cones = np.stack([pick(), pick()], axis=1)
    return _rows(sc, rng, n, (0, 0, 0, 1), None, cones=cones, cos=(3.0e-4, 1.0), dist=(1.0e-3, 1.0e3), log_dist=True, back=0.2)


WRAPS = ["wrap%d%d%d" % (ws, wt, linear) for ws in range(3) for wt in range(3) for linear in (True, False)]
CLASSES = {
    "tangent/vertex": _geometry("vertex", (0, 1)),
    "tangent/none": _geometry("none_mixed", (0, 0, 1, 2, 3)),
    "tangent/none-at-all": _geometry("none", (0, 1)),
    "tangent/untrusted": _geometry("untrusted", (0, 1, 2)),
    # one class per angle: the basis of a tangent a rad from the normal carries float32's cancellation, 1e-7 / a, and so does its bound
    **{"tangent/parallel-%.1e" % a: _geometry("parallel", (i,)) for i, a in enumerate(PARALLEL)},
    "tangent/degenerate-uv": _geometry("degenerate_uv", (0, 1, 2, 3, 4), back=0.3),
    "transform/mirrored": _geometry("mirrored", (0, 1, 2, 3), back=0.2),
    "transform/sheared": _geometry("sheared", (0, 1, 2), back=0.2),
    "side/back": _geometry("vertex", (0, 1), ("all", "all_one_sided", "normal_only"), back=1.0),
    "normal/zero": _geometry("normal_zero", (0, 1, 2), back=0.3),
    "bary/edges": _geometry("vertex", (0, 1), bary="edges"),
    "material/slots": _material(["slot%d" % s for s in range(6)] + ["all"]),
    "material/uv-sets": _material(["uvset1", "uvset2", "uvset7", "normal_uv1"]),
    "material/transforms": _material(["xf_rot", "xf_zero", "xf_nan", "xf_inf"]),
    "material/wraps": _material(WRAPS),
    "material/orm": _material(["orm_shared", "orm_shared_off"]),
    "material/texture-index": _material(["tex_at_count", "tex_past_count"]),
    "material/factors": _material(["factors_a", "factors_b"]),
    "material/normal-scale": _material(["nscale%d" % i for i in range(6)]),
    # (a third from behind: texels that tip the mapped normal below the surface turn it on either side)
    "material/normal-texels": _material(["n_half", "n_zero", "n_one", "n_short", "n_half_x2", "n_zero_x2", "n_one_x2", "n_short_x2"], back=0.3),
    "material/emissive": _material(["emissive_hot"]),
    "material/alpha": _material(["opaque", "mask", "mask_factor", "blend"]),
    "material/nearest": _material(["near33", "near16"]),
    "material/not-pbr": _material(["lambert"]),
    "footprint": ("footprint", _footprint),
}
GROUPS = {"tangent": [c for c in CLASSES if c.startswith("tangent/")],
          "transform-side-bary": [c for c in CLASSES if c.split("/")[0] in ("transform", "side", "normal", "bary")],
          "material": [c for c in CLASSES if c.startswith("material/")],
          "footprint": ["footprint"]}


def class_rows(name):
    """(scene, rows [ROWS, 20]) of a class; the same rows on every call."""
    scene_name, make = CLASSES[name]
    sc = scene(scene_name)
    seed = int.from_bytes(name.encode(), "little") % (2 ** 32)
    return sc, make(sc, np.random.default_rng(seed))


def gradient_rows(rng, rows):
    """The rows as instantiation 1 with gradients of their own: nearly isotropic (1:1.02 .. 1:1.5), 1:2 .. 1:20 anisotropic along
    either axis, zero, and too large for the variance term (gradMag >= 4); one set valid, the other, or both.  An exactly isotropic
    footprint has Pmax / Pmin = 1 up to rounding and sits on the threshold of ceil(Pmax / Pmin) itself (one tap or two): every such row
    would be guarded, so none is drawn."""
    n = rows.shape[0]
    grads = np.zeros((n, 8))
    for s in (0, 1):
        kind = rng.integers(0, 5, size=n)
        theta = rng.uniform(0.0, 2.0 * np.pi, size=n)
        size = 10.0 ** rng.uniform(-3.0, -0.5, size=n)
        size = np.where(kind == 4, rng.uniform(4.0, 40.0, size=n), size)
        ratio = np.where((kind == 1) | (kind == 2), rng.uniform(2.0, 20.0, size=n), rng.uniform(1.02, 1.5, size=n))
        major = np.stack([np.cos(theta), np.sin(theta)], axis=1) * size[:, None]
        minor = np.stack([-np.sin(theta), np.cos(theta)], axis=1) * (size / ratio)[:, None]
        gx, gy = np.where((kind == 2)[:, None], minor, major), np.where((kind == 2)[:, None], major, minor)
        g = np.concatenate([gx, gy], axis=1)
        grads[:, 4 * s:4 * s + 4] = np.where((kind == 3)[:, None], 0.0, g)
    out = rows.copy()
    out[:, 11:19] = grads.astype(f32)
    w = out.view(np.uint32)
    w[:, 10] = 1
    w[:, 19] = rng.integers(1, 4, size=n).astype(np.uint32)
    return out


GRADIENT_MATERIALS = ["all", "xf_rot", "uvset1", "near33", "near16", "normal_uv1", "n_short", "mask", "blend"]


def gradient_class_rows():
    """grad/given: (scene, rows) on the geometry of tangent/vertex, through a rotated texture transform and on NEAREST textures."""
    sc = scene("vertex")
    rng = np.random.default_rng(77)
    return sc, gradient_rows(rng, _rows(sc, rng, ROWS, (0, 1), GRADIENT_MATERIALS))


# --------------------------------------------------------------------------------------------- comparison
COLOURS, SCALARS = ("base_color", "emissive"), ("roughness", "metallic", "transmission", "occlusion")


def angle(a, b):
    """The angle between unit vectors, from the chord (well conditioned near 0)."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return 2.0 * np.arcsin(np.clip(np.linalg.norm(a - b, axis=-1) / 2.0, 0.0, 1.0))


def differences(ref, got):
    """Largest differences of `got` (probe fields) from the reference on the rows that are hit, textured on both sides, kept on both
    sides and not guarded: {"colour", "scalar", "normal"} (normal: the angle), the rows compared and guarded, and the rows whose
    branch outcomes differ (discard, basis and flip, random state, two-sided) among the unguarded ones."""
    hit = np.asarray(got["hit"]) > 0
    near = guarded(ref)
    textured = hit & ref["textured"]
    use = textured & ~near
    branch = hit & (ref["textured"] != (got["textured"] > 0))   # (every hit row: also one the reference alone calls untextured)
    branch |= use & ((ref["discard"] != (got["discard"] > 0)) | (ref["state"] != got["state"]))
    kept = use & ~ref["discard"] & ~(got["discard"] > 0)
    branch |= kept & ((ref["basis"] != got["basis"]) | (ref["two_sided"] != (got["two_sided"] > 0)))
    res = {"rows": int(hit.sum()), "textured": int(textured.sum()), "guarded": int((textured & near).sum()), "compared": int(kept.sum()),
           "branch_mismatches": np.nonzero(branch)[0], "colour": 0.0, "scalar": 0.0, "normal": 0.0, "range": {"colour": 1.0, "scalar": 1.0}}
    if kept.any():
        res["colour"] = max(float(np.abs(ref[f][kept] - got[f][kept]).max()) for f in COLOURS)
        res["scalar"] = max(float(np.abs(ref[f][kept] - got[f][kept]).max()) for f in SCALARS)
        res["normal"] = float(angle(ref["normal"][kept], got["normal"][kept]).max())
        res["range"] = {"colour": max(1.0, max(float(np.abs(ref[f][kept]).max()) for f in COLOURS)), "scalar": 1.0}
    return res


def bounds(name, ranges=None):
    """What the device may differ from the reference by in class `name`: 4 x the oracle's own largest difference, and no less than
    4 float32 ulps of the output's range (the normal: of a unit vector's component)."""
    ranges = ranges or {"colour": 1.0, "scalar": 1.0}
    m = ORACLE_MEASURED[name]
    return {"colour": max(4.0 * m["colour"], 4.0 * EPS32 * ranges["colour"]), "scalar": max(4.0 * m["scalar"], 4.0 * EPS32),
            "normal": max(4.0 * m["normal"], 4.0 * EPS32)}


# The oracle's largest absolute difference from the reference on the unguarded rows of each class (the normal: the angle in radians),
# as tests/test_pbr_hit_host.py recomputes it; a recomputed value above the one here fails that test.
ORACLE_MEASURED = {
    "tangent/vertex": {"colour": 5.0e-06, "scalar": 3.0e-06, "normal": 4.9e-06},
    "tangent/none": {"colour": 9.7e-06, "scalar": 2.9e-06, "normal": 1.1e-05},
    "tangent/none-at-all": {"colour": 8.2e-07, "scalar": 3.3e-06, "normal": 1.8e-05},
    "tangent/untrusted": {"colour": 1.3e-05, "scalar": 5.2e-06, "normal": 1.2e-05},
    # the projection of a unit tangent a rad from the normal is a long and carries float32's absolute rounding of 1e-7: 1e-7 / a rad
    "tangent/parallel-1.0e-04": {"colour": 7.8e-07, "scalar": 2.0e-06, "normal": 1.2e-03},
    "tangent/parallel-3.0e-04": {"colour": 2.8e-06, "scalar": 1.3e-06, "normal": 3.4e-04},
    "tangent/parallel-6.0e-04": {"colour": 1.5e-06, "scalar": 1.3e-06, "normal": 1.3e-04},
    "tangent/parallel-1.5e-03": {"colour": 1.2e-06, "scalar": 1.9e-06, "normal": 6.8e-05},
    "tangent/parallel-4.0e-03": {"colour": 1.0e-05, "scalar": 2.7e-06, "normal": 2.3e-05},
    "tangent/parallel-1.0e-02": {"colour": 1.4e-05, "scalar": 7.3e-06, "normal": 1.5e-05},
    "tangent/degenerate-uv": {"colour": 5.5e-07, "scalar": 3.9e-06, "normal": 1.8e-05},
    "transform/mirrored": {"colour": 1.5e-05, "scalar": 8.2e-06, "normal": 1.8e-05},
    "transform/sheared": {"colour": 1.1e-05, "scalar": 3.6e-06, "normal": 6.5e-06},
    "side/back": {"colour": 4.3e-06, "scalar": 3.5e-06, "normal": 4.6e-06},
    "normal/zero": {"colour": 5.3e-06, "scalar": 3.2e-06, "normal": 6.9e-06},
    "bary/edges": {"colour": 4.3e-06, "scalar": 2.7e-06, "normal": 4.5e-06},
    "material/slots": {"colour": 3.3e-06, "scalar": 3.2e-06, "normal": 4.3e-06},
    "material/uv-sets": {"colour": 5.9e-06, "scalar": 2.9e-06, "normal": 9.8e-06},
    "material/transforms": {"colour": 5.6e-06, "scalar": 3.8e-06, "normal": 9.5e-06},
    "material/wraps": {"colour": 3.0e-06, "scalar": 6.0e-10, "normal": 1.8e-07},
    "material/orm": {"colour": 0.0e+00, "scalar": 3.7e-06, "normal": 1.8e-07},
    "material/texture-index": {"colour": 0.0e+00, "scalar": 6.0e-10, "normal": 1.8e-07},
    "material/factors": {"colour": 7.7e-06, "scalar": 4.2e-06, "normal": 9.5e-06},
    "material/normal-scale": {"colour": 0.0e+00, "scalar": 4.6e-06, "normal": 2.1e-05},
    "material/normal-texels": {"colour": 0.0e+00, "scalar": 6.5e-07, "normal": 5.3e-06},
    "material/emissive": {"colour": 7.7e-06, "scalar": 0.0e+00, "normal": 1.8e-07},
    "material/alpha": {"colour": 2.7e-06, "scalar": 6.0e-10, "normal": 1.8e-07},
    "material/nearest": {"colour": 5.6e-08, "scalar": 7.1e-07, "normal": 4.3e-06},
    "material/not-pbr": {"colour": 0.0e+00, "scalar": 0.0e+00, "normal": 0.0e+00},
    "footprint": {"colour": 1.5e-05, "scalar": 1.5e-05, "normal": 2.1e-05},
}
