"""GPU tests of the first-hit ray differentials of the textured Metal path (PTR_METAL_RAY_DIFF, include/ptr_abi.h bit 8).

The scenes are built from numpy arrays (the builder of tests/pbr_hit_domain.py): quads with known vertices and uvs and small generated textures.  The restatements of the
rule are in this file: the gradients in float64 and the anisotropic filter of csrc/kernels/texture.h in float32.  The filter reads a mip
chain taken from ptr_debug_env_mips, which uses the same chain rule.
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import oracle_lib as ol
import pbr_hit_domain as D

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(ROOT, "scenes")

pytestmark = pytest.mark.gpu

RAY_DIFF = pt.PTR_METAL_RAY_DIFF
PBR = pt.PTR_METAL_PBR
ENV_LOD = pt.PTR_METAL_ENV_LOD
NO_TEX = 0xFFFFFFFF
f32 = np.float32

SETTINGS_SCENE = """camera target=0,0,0 distance=6 yaw=1.5707963 pitch=0.5 vfov=40
renderer width=64 height=48 maxDepth=1 seed=1337
background solid=0,0,0
material type=lambert albedo=0.5,0.5,0.5 name=m
sphere center=0,-1000,0 radius=0.001 material=0
"""


def _with(s, **kw):
    s = s.copy()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _settings(tmp_path, **kw):
    p = tmp_path / "settings.scene"
    p.write_text(SETTINGS_SCENE)
    host = pt.HostScene.load(str(p), SCENES)
    s = host.settings_for(width=kw.pop("width", 64), height=kw.pop("height", 48), max_depth=1, seed=1337)
    return _with(s, **kw)


# The scene builder is shared with the per-hit material classes (tests/pbr_hit_domain.py), which extend it with normals, tangents and
# localToWorld
Texture, Scene, _pbr_material = D.Texture, D.Scene, D.pbr_material


def _ground(x0, x1, z0, z1, uv_of, material=0, uv1_of=None):
    """Quad on y = 0: two triangles (v0, v1, v2), (v0, v2, v3); uv_of(x, z) -> (u, v)."""
    p = np.array([[x0, 0.0, z0], [x1, 0.0, z0], [x1, 0.0, z1], [x0, 0.0, z1]], np.float64)
    uv0 = np.array([uv_of(x, z) for x, _, z in p])
    uv1 = np.array([(uv1_of or uv_of)(x, z) for x, _, z in p])
    return {"positions": p, "indices": np.array([[0, 1, 2], [0, 2, 3]]), "uv0": uv0, "uv1": uv1, "material": material}


# --------------------------------------------------------------------------- restatements
def _partials64(p0, p1, p2, q0, q1, q2):
    """triangle_surface_partials (shaders/pathtrace.metal:741-820) in float64, with its area fallback; None when it fails."""
    e1, e2 = p1 - p0, p2 - p0
    d1, d2 = q1 - q0, q2 - q0
    det = d1[0] * d2[1] - d1[1] * d2[0]
    if abs(det) > 1e-9:
        dpdu = (e1 * d2[1] - e2 * d1[1]) / det
        dpdv = (e2 * d1[0] - e1 * d2[0]) / det
        if np.linalg.norm(dpdu) > 1e-8 and np.linalg.norm(dpdv) > 1e-8:
            return dpdu, dpdv
    world, uv = np.linalg.norm(np.cross(e1, e2)), abs(det)
    if not (world > 1e-12 and uv > 1e-12):
        return None
    per = np.sqrt(uv / world)
    t = e1 / np.linalg.norm(e1)
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n)
    b = np.cross(n, t)
    b /= np.linalg.norm(b)
    return t / per, b / per


def _restated_grads(cam, width, height, mesh, rays):
    """Points 1-2 of the rule in float64 for rays (origin, unit direction) that hit the quad `mesh` (y = 0): per ray (t, grads of uv
    set 0, grads of uv set 1, valid 0, valid 1), grads = (dudx, dvdx, dudy, dvdy)."""
    origin, lower_left, horizontal, vertical = (cam[0:3].astype(np.float64), cam[3:6].astype(np.float64), cam[6:9].astype(np.float64),
                                                cam[9:12].astype(np.float64))
    c = np.cross(horizontal, vertical)
    ddx, ddy = horizontal / width, -vertical / height
    P = mesh["positions"]
    out = []
    for o, D in rays.astype(np.float64):
        D = D / np.linalg.norm(D)
        t = -o[1] / D[1]
        hit = o + t * D
        # triangle 0 = (v0, v1, v2) covers x - x0 >= ... : decide by the side of the diagonal v0 -> v2
        diag = P[2] - P[0]
        side = np.cross(diag, hit - P[0])[1] * np.cross(diag, P[1] - P[0])[1]
        tri = mesh["indices"][0] if side >= 0 else mesh["indices"][1]
        N = np.array([0.0, 1.0, 0.0])
        dlen = np.dot(lower_left - origin, c) / np.dot(D, c)
        s = t / dlen
        nd = np.dot(N, D)
        dpdx = s * (ddx - np.dot(N, ddx) / nd * D)
        dpdy = s * (ddy - np.dot(N, ddy) / nd * D)
        row = [t]
        valid = []
        for key in ("uv0", "uv1"):
            q = mesh[key].astype(np.float64)
            part = _partials64(P[tri[0]], P[tri[1]], P[tri[2]], q[tri[0]], q[tri[1]], q[tri[2]])
            if part is None or abs(dlen * nd) < 1e-6:
                row.extend([0.0] * 4)
                valid.append(0.0)
                continue
            dpdu, dpdv = part
            a00, a01, a11 = dpdu @ dpdu, dpdu @ dpdv, dpdv @ dpdv
            det = a00 * a11 - a01 * a01
            dudp, dvdp = (a11 * dpdu - a01 * dpdv) / det, (a00 * dpdv - a01 * dpdu) / det
            row.extend([dudp @ dpdx, dvdp @ dpdx, dudp @ dpdy, dvdp @ dpdy])
            valid.append(1.0)
        out.append(row + valid)
    return np.array(out)


def _wrap(i, n, mode):
    if mode == 1:
        return np.clip(i, 0, n - 1)
    if mode == 2:
        j = np.mod(i, 2 * n)
        return np.where(j < n, j, 2 * n - 1 - j)
    return np.mod(i, n)


def _bilinear(tex, level, u, v):
    img = tex.levels[level]
    H, W = img.shape[:2]
    if not tex.linear:
        x = _wrap(np.floor(u * f32(W)).astype(np.int64), W, tex.wrap_s)
        y = _wrap(np.floor(v * f32(H)).astype(np.int64), H, tex.wrap_t)
        return img[y, x]
    fx, fy = (u * f32(W) - f32(0.5)).astype(f32), (v * f32(H) - f32(0.5)).astype(f32)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0f)[:, None], (fy - y0f)[:, None]
    x0i, y0i = x0f.astype(np.int64), y0f.astype(np.int64)
    x0, x1 = _wrap(x0i, W, tex.wrap_s), _wrap(x0i + 1, W, tex.wrap_s)
    y0, y1 = _wrap(y0i, H, tex.wrap_t), _wrap(y0i + 1, H, tex.wrap_t)
    ix, iy = f32(1) - tx, f32(1) - ty
    return (img[y0, x0] * ix + img[y0, x1] * tx) * iy + (img[y1, x0] * ix + img[y1, x1] * tx) * ty


def _level_sample(tex, u, v, lod):
    """texTaps with one tap: bilinear per level, linear between the two nearest levels; NEAREST: the rounded level."""
    u, v, lod = np.asarray(u, f32), np.asarray(v, f32), np.asarray(lod, f32)
    n = len(tex.levels)
    l = np.clip(lod, f32(0), f32(n - 1))
    out = np.zeros((len(u), 4), f32)
    if not tex.linear:
        lvl = np.floor(l + f32(0.5)).astype(np.int64)
        for k in range(n):
            idx = lvl == k
            if idx.any():
                out[idx] = _bilinear(tex, k, u[idx], v[idx])
        return out
    l0 = np.floor(l).astype(np.int64)
    frac = (l - np.floor(l)).astype(f32)
    for k in range(n):
        idx = l0 == k
        if not idx.any():
            continue
        a = _bilinear(tex, k, u[idx], v[idx])
        if k + 1 < n:
            fr = frac[idx]
            mix = fr > 0
            if mix.any():
                b = _bilinear(tex, k + 1, u[idx][mix], v[idx][mix])
                a[mix] = a[mix] + (b - a[mix]) * fr[mix][:, None]
        out[idx] = a
    return out


def _grad_sample(tex, q):
    """Point 6 (csrc/kernels/texture.h texAniso + texTaps) in float32: q [n, 6] {u, v, dudx, dvdx, dudy, dvdy} -> (RGBA, Nt)."""
    q = np.asarray(q, f32)
    u, v, dudx, dvdx, dudy, dvdy = q.T
    H, W = tex.rgba.shape[:2]
    n = len(tex.levels)
    xw, xh, yw, yh = dudx * f32(W), dvdx * f32(H), dudy * f32(W), dvdy * f32(H)
    px, py = np.sqrt(xw * xw + xh * xh), np.sqrt(yw * yw + yh * yh)
    xmaj = px >= py
    pmax, pmin = np.where(xmaj, px, py), np.where(xmaj, py, px)
    A = f32(8) if (tex.linear and n > 1) else f32(1)
    nt = np.maximum(np.minimum(np.ceil(pmax / np.maximum(pmin, f32(1e-6))), A), f32(1)).astype(f32)
    with np.errstate(divide="ignore"):
        lod = np.clip(np.log2(pmax / nt), f32(0), f32(n - 1)).astype(f32)
    gu, gv = np.where(xmaj, dudx, dudy), np.where(xmaj, dvdx, dvdy)
    if not tex.linear:
        return _level_sample(tex, u, v, lod), nt
    total = np.zeros((len(u), 4), f32)
    for i in range(8):
        idx = i < nt
        if not idx.any():
            break
        o = ((f32(i) + f32(0.5)) / nt[idx] - f32(0.5)).astype(f32)
        total[idx] = total[idx] + _level_sample(tex, u[idx] + o * gu[idx], v[idx] + o * gv[idx], lod[idx])
    return (total / nt[:, None]).astype(f32), nt


def _pixel_xys(width, height, spp):
    ys, xs, ss = np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), ss.ravel()], axis=1).astype(np.uint32)


def _random_texture(rng, w, h, wrap_s=0, wrap_t=0, linear=True):
    return Texture(rng.uniform(0.05, 1.0, size=(h, w, 4)).astype(np.float32), wrap_s, wrap_t, linear)


# --------------------------------------------------------------------------- 1. gradients
@pytest.mark.parametrize("lens", [False, True])
def test_first_hit_gradients_match_restatement(tmp_path, lens):
    rng = np.random.default_rng(11)
    c, s = np.cos(0.3), np.sin(0.3)
    rows = ((1.5 * c, -0.7 * s, 0.2), (1.5 * s, 0.7 * c, -0.1))   # KHR_texture_transform of the base-colour slot (uv set 1)
    mesh = _ground(-3.0, 2.5, -4.0, 3.0, lambda x, z: (0.21 * x + 0.05 * z + 0.3, -0.03 * x + 0.17 * z), uv1_of=lambda x, z: (0.5 * z - 0.1 * x, 0.9 * x))
    tex = _random_texture(rng, 32, 32)
    mat = _pbr_material(textures={0: 0}, uv_sets={0: 1}, transforms={0: rows})
    scene = Scene([mesh], [mat], [tex])
    st = _settings(tmp_path, width=64, height=48)
    if lens:
        st = _with(st, cameraDefocusAngle=3.0, cameraFocusDistance=5.0)
    st = _with(st, metalSemantics=PBR | RAY_DIFF)
    cam = ol.build_camera(st)
    assert (cam[18] > 0) == lens
    xys = _pixel_xys(64, 48, 2)[::7]
    rays, _ = pt.debug_camera_rays(st, xys)
    got = scene.dev.first_hit_textures(st, xys)
    hit = got["textured"] > 0
    assert hit.mean() > 0.5
    want = _restated_grads(cam, 64.0, 48.0, mesh, np.stack([rays[hit][:, 0:3], rays[hit][:, 3:6]], axis=1))
    assert np.allclose(got["t"][hit], want[:, 0], rtol=1e-5)
    assert (got["valid0"][hit] == 1).all() and (got["valid1"][hit] == 1).all()
    for key, cols in (("grad0", slice(1, 5)), ("grad1", slice(5, 9))):
        g, w = got[key][hit].astype(np.float64), want[:, cols]
        scale = np.abs(w).max(axis=1, keepdims=True)
        assert np.allclose(g, w, rtol=1e-4, atol=1e-4 * scale), (key, np.abs(g - w).max())
    # point 3: the base-colour slot's gradients through the transform's linear part
    L = np.array([[rows[0][0], rows[0][1]], [rows[1][0], rows[1][1]]])
    g1 = want[:, 5:9]
    base = np.concatenate([g1[:, 0:2] @ L.T, g1[:, 2:4] @ L.T], axis=1)
    gb = got["base_grad"][hit].astype(np.float64)
    assert (got["base_valid"][hit] == 1).all()
    assert np.allclose(gb, base, rtol=1e-4, atol=1e-4 * np.abs(base).max(axis=1, keepdims=True))
    # without the bit: no gradients anywhere
    off = scene.dev.first_hit_textures(_with(st, metalSemantics=PBR), xys)
    assert (off["valid0"] == 0).all() and (off["valid1"] == 0).all() and (off["grad0"] == 0).all()


def test_degenerate_uv_sets_fall_back_or_drop_the_gradients(tmp_path):
    rng = np.random.default_rng(12)
    # uv set 0: |det| = 4e-10 per triangle (|det| <= 1e-9): the area fallback of triangle_surface_partials; uv set 1: one point
    mesh = _ground(-2.0, 2.0, -2.0, 2.0, lambda x, z: (5e-6 * x, 5e-6 * z), uv1_of=lambda x, z: (0.25, 0.5))
    scene = Scene([mesh], [_pbr_material(textures={0: 0})], [_random_texture(rng, 16, 16)])
    st = _with(_settings(tmp_path, width=48, height=32), metalSemantics=PBR | RAY_DIFF)
    xys = _pixel_xys(48, 32, 1)[::5]
    rays, _ = pt.debug_camera_rays(st, xys)
    got = scene.dev.first_hit_textures(st, xys)
    hit = got["textured"] > 0
    assert hit.mean() > 0.3
    want = _restated_grads(ol.build_camera(st), 48.0, 32.0, mesh, np.stack([rays[hit][:, 0:3], rays[hit][:, 3:6]], axis=1))
    assert (want[:, 9] == 1).all() and (want[:, 10] == 0).all()
    assert (got["valid0"][hit] == 1).all() and (got["valid1"][hit] == 0).all() and (got["grad1"][hit] == 0).all()
    g, w = got["grad0"][hit].astype(np.float64), want[:, 1:5]
    assert np.allclose(g, w, rtol=1e-4, atol=1e-4 * np.abs(w).max(axis=1, keepdims=True)), np.abs(g - w).max()


# --------------------------------------------------------------------------- 2. the filter
@pytest.mark.parametrize("wrap,linear", [(0, True), (2, True), (1, True), (0, False)])
def test_gradient_sample_matches_restatement(tmp_path, wrap, linear):
    rng = np.random.default_rng(20 + wrap + 4 * int(linear))
    tex = _random_texture(rng, 64, 64, wrap, wrap, linear)
    scene = Scene([_ground(-1, 1, -1, 1, lambda x, z: (x, z))], [_pbr_material(textures={0: 0})], [tex])
    rows = []
    for k in range(1, 11):                 # Nt = 1 (isotropic) ... 8, then clamped at 8
        ratio = 1.0 if k == 1 else k - 0.5
        for _ in range(24):
            minor = rng.uniform(0.2, 6.0) / 64.0   # in uv; x 64 texels
            ang = rng.uniform(0, 2 * np.pi)
            ax, ay = np.cos(ang), np.sin(ang)
            if k == 1:
                gx, gy = (minor, 0.0), (0.0, minor)
            else:
                gx, gy = (minor * ratio * ax, minor * ratio * ay), (-minor * ay, minor * ax)
            if rng.uniform() < 0.5:
                gx, gy = gy, gx
            rows.append([rng.uniform(-1.5, 2.5), rng.uniform(-1.5, 2.5), gx[0], gx[1], gy[0], gy[1]])
    q = np.array(rows, np.float32)
    got = scene.dev.texture_sample_grad(0, q)
    want, nt = _grad_sample(tex, q)
    if linear:
        assert set(np.unique(nt).astype(int)) == set(range(1, 9))
    else:
        assert (nt == 1).all()
    assert np.allclose(got, want, rtol=1e-4, atol=2e-6), np.abs(got - want).max()
    # a texture index that does not exist reads the fallback
    assert (scene.dev.texture_sample_grad(5, q[:3]) == -1).all()


# --------------------------------------------------------------------------- 3. the image: a grazing striped floor
def _stripes_scene():
    W, H = 16, 4
    img = np.zeros((H, W, 4), np.float32)
    img[:, 0::2, :3] = 0.9
    img[:, 1::2, :3] = 0.1
    img[..., 3] = 1.0
    tex = Texture(img, 0, 0, True)
    # u across the view (0.4 world units per texel), v along the view (100 world units per texture height: short footprints in v)
    mesh = _ground(-40.0, 40.0, -200.0, 4.0, lambda x, z: (x / 6.4, z / 100.0))
    mat = _pbr_material(base=(0.0, 0.0, 0.0), roughness=1.0, emission=(1.0, 1.0, 1.0), textures={4: 0})
    return Scene([mesh], [mat], [tex]), tex, mesh


def test_grazing_stripes_follow_the_anisotropic_rule(tmp_path):
    scene, tex, _ = _stripes_scene()
    width, height, spp = 128, 96, 4
    st = _settings(tmp_path, width=width, height=height)
    st = _with(st, cameraTarget=(C.c_float * 3)(0.0, 0.0, -10.0), cameraDistance=10.0, cameraYaw=float(np.pi / 2), cameraPitch=0.06,
               cameraVerticalFov=30.0, maxDepth=1, metalSemantics=PBR | RAY_DIFF)
    on, _ = scene.dev.render_image(st, spp)
    off, _ = scene.dev.render_image(_with(st, metalSemantics=PBR), spp)
    xys = _pixel_xys(width, height, spp)
    got = scene.dev.first_hit_textures(st, xys)
    hit = got["textured"] > 0
    assert (got["valid0"][hit] == 1).all()
    value = np.zeros((len(xys), 3), np.float32)
    q = np.concatenate([got["uv0"][hit], got["grad0"][hit]], axis=1)
    value[hit] = _grad_sample(tex, q)[0][:, :3]
    want = value.reshape(height, width, spp, 3).astype(np.float64).mean(axis=2)
    close = np.isclose(on, want, rtol=1e-3, atol=1e-5).all(axis=2)
    assert close.mean() >= 0.99, close.mean()
    # far field: the rows whose every sample hits the floor more than 15 units away
    t = got["t"].reshape(height, width, spp)
    far = ((t > 15.0) & hit.reshape(height, width, spp)).all(axis=(1, 2))
    assert far.sum() >= 3
    contrast_on = float(on[far, :, 0].std(axis=1).mean())
    contrast_off = float(off[far, :, 0].std(axis=1).mean())
    assert contrast_on > 0.05 and contrast_on > 4.0 * contrast_off, (contrast_on, contrast_off)


# --------------------------------------------------------------------------- 4. normal variance
def _decode(s, scale):
    n = s[:, :3].astype(f32) * f32(2) - f32(1)
    n[:, 0] *= f32(scale)
    n[:, 1] *= f32(scale)
    length = np.sqrt((n * n).sum(axis=1, dtype=f32))
    n[:, 2] = np.sqrt(np.maximum(f32(1) - (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]), f32(0)))
    n = n / np.sqrt((n * n).sum(axis=1, dtype=f32))[:, None]
    return n.astype(f32), length.astype(f32)


def test_normal_variance_widens_the_roughness(tmp_path):
    rng = np.random.default_rng(31)
    H = W = 32
    nrm = np.empty((H, W, 4), np.float32)
    nrm[..., 0] = rng.uniform(0.3, 0.7, (H, W))
    nrm[..., 1] = rng.uniform(0.3, 0.7, (H, W))
    nrm[..., 2] = 1.0
    nrm[..., 3] = 1.0
    tex = Texture(nrm, 0, 0, True)
    scale, rough = 0.8, 0.3
    mesh = _ground(-3.0, 3.0, -6.0, 3.0, lambda x, z: (x / 2.0, z / 2.0))
    scene = Scene([mesh], [_pbr_material(roughness=rough, textures={2: 0}, normal_scale=scale)], [tex])
    st = _with(_settings(tmp_path, width=64, height=48), metalSemantics=PBR | RAY_DIFF)
    xys = _pixel_xys(64, 48, 1)[::3]
    got = scene.dev.first_hit_textures(st, xys)
    hit = got["textured"] > 0
    assert hit.mean() > 0.5 and (got["valid0"][hit] == 1).all()
    uv, g = got["uv0"][hit], got["grad0"][hit]
    ns, _ = _grad_sample(tex, np.concatenate([uv, g], axis=1))
    n, length = _decode(ns, scale)
    tok = np.maximum((f32(1) - length) / np.maximum(length, f32(1e-6)), f32(0))
    mag = np.abs(g).max(axis=1)
    rho = np.maximum(np.maximum(np.abs(g[:, 0]) * W, np.abs(g[:, 1]) * H), np.maximum(np.abs(g[:, 2]) * W, np.abs(g[:, 3]) * H)).astype(f32)
    assert (rho > 0).all()
    lod = np.clip(np.log2(np.maximum(rho, f32(1e-8))), f32(0), f32(len(tex.levels) - 1)).astype(f32)
    dx, _ = _decode(_level_sample(tex, uv[:, 0] + g[:, 0], uv[:, 1] + g[:, 1], lod), scale)
    dy, _ = _decode(_level_sample(tex, uv[:, 0] + g[:, 2], uv[:, 1] + g[:, 3], lod), scale)
    var = np.maximum(np.maximum(f32(1) - (n * dx).sum(axis=1, dtype=f32), f32(0)), np.maximum(f32(1) - (n * dy).sum(axis=1, dtype=f32), f32(0)))
    widen = (mag > 1e-6) & (mag < 4.0)
    assert widen.mean() > 0.9
    tok = tok + np.where(widen, f32(0.35) * var, f32(0))
    want = np.clip(np.sqrt(f32(rough) * f32(rough) + tok), 0, 1)
    assert np.allclose(got["roughness"][hit], want, rtol=1e-3, atol=1e-5), np.abs(got["roughness"][hit] - want).max()
    off = scene.dev.first_hit_textures(_with(st, metalSemantics=PBR), xys)
    assert (got["roughness"][hit] > off["roughness"][hit] + 1e-4).mean() > 0.5   # the variance term shows


# --------------------------------------------------------------------------- 5. no change where none is due
def test_the_bit_changes_nothing_without_a_first_hit_texture_lookup(tmp_path):
    from scenes.gen_assets import ensure_assets

    ensure_assets()
    host = pt.HostScene.load(os.path.join(GOLDEN, "env_materials.scene"), SCENES)   # untextured
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for(width=64, height=48, max_depth=6, seed=1337)
    for base in (0, 127, 127 | ENV_LOD):
        a, _ = dev.render_image(_with(s, metalSemantics=base), 4)
        b, _ = dev.render_image(_with(s, metalSemantics=base | RAY_DIFF), 4)
        assert a.mean() > 0.01 and np.array_equal(a, b), base
        ia, sa = dev.render_signatures(_with(s, metalSemantics=base))
        ib, sb = dev.render_signatures(_with(s, metalSemantics=base | RAY_DIFF))
        assert np.array_equal(ia, ib) and np.array_equal(sa, sb), base
    host = pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN)        # textured, without PBR
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for(width=64, height=48, max_depth=4, seed=1337)
    for base in (0, 127 & ~PBR, (127 & ~PBR) | ENV_LOD):
        a, _ = dev.render_image(_with(s, metalSemantics=base), 4)
        b, _ = dev.render_image(_with(s, metalSemantics=base | RAY_DIFF), 4)
        assert a.mean() > 0.01 and np.array_equal(a, b), base
        ia, sa = dev.render_signatures(_with(s, metalSemantics=base))
        ib, sb = dev.render_signatures(_with(s, metalSemantics=base | RAY_DIFF))
        assert np.array_equal(ia, ib) and np.array_equal(sa, sb), base
    with_pbr, _ = dev.render_image(_with(s, metalSemantics=127), 4)
    with_bit, _ = dev.render_image(_with(s, metalSemantics=127 | RAY_DIFF), 4)
    assert not np.array_equal(with_pbr, with_bit)   # ... and with PBR it does change the textured scene


def test_a_linear_ramp_changes_only_by_rounding(tmp_path):
    ramp = np.zeros((4, 64, 4), np.float32)
    ramp[..., 0] = ((np.arange(64) + 0.5) / 64.0)[None, :]
    ramp[..., 1] = 0.5
    ramp[..., 2] = 1.0 - ramp[..., 0]
    ramp[..., 3] = 1.0
    tex = Texture(ramp, 1, 1, True)
    # u in [0.3, 0.7] across the floor, far from the clamped borders
    # (an oblique view, not a grazing one: the cone's LOD stays below the 1x1 level, whose one texel is no longer the ramp)
    mesh = _ground(-6.0, 6.0, -6.0, 6.0, lambda x, z: (0.5 + x / 30.0, 0.5 + z / 1000.0))
    scene = Scene([mesh], [_pbr_material(base=(0.0, 0.0, 0.0), emission=(1.0, 1.0, 1.0), textures={4: 0})], [tex])
    st = _with(_settings(tmp_path, width=96, height=48), metalSemantics=PBR)
    off, _ = scene.dev.render_image(st, 4)
    on, _ = scene.dev.render_image(_with(st, metalSemantics=PBR | RAY_DIFF), 4)
    assert off.mean() > 0.05
    assert np.allclose(on, off, rtol=2e-5, atol=2e-6), float(np.abs(on - off).max())


# --------------------------------------------------------------------------- 6. scheduling
def test_scheduling_does_not_show(tmp_path):
    host = pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN)
    s = _with(host.settings_for(width=512, height=512, max_depth=4, seed=1337), metalSemantics=127 | RAY_DIFF)

    def render(env):
        os.environ.update(env)       # the knobs are read when the scene is uploaded
        try:
            dev = pt.DeviceScene(host.desc, 0, keepalive=host)
            image, _ = dev.render_image(s, 16)
            dev.close()
        finally:
            for k in env:
                del os.environ[k]
        return image

    ref = render({})
    assert ref.mean() > 0.01
    for env in ({"PTR_POOL_GROUPS": "1"}, {"PTR_POOL_GROUPS": "4"}, {"PTR_CONNECT_OVERLAP": "0"}, {"PTR_TAIL_BELOW": "0"},
                {"PTR_POOL_SLOTS": str(3 << 18), "PTR_REFILL_BELOW": "24"}, {"PTR_MAX_ITEMS": str(512 * 512 * 16)}):
        assert np.array_equal(render(env), ref), env
    parts = [pt.DeviceScene(host.desc, 0, keepalive=host).render(s, 16, part=p, parts=3)[0] for p in range(3)]
    assert np.array_equal(pt.assemble_bands(parts, 512, 512), ref)
