"""GPU tests of the prefiltered environment lookups of the Metal kernel (PTR_METAL_ENV_LOD, include/ptr_abi.h).

The oracle restates the level-0 lookups only.  The image-level check therefore goes through a map whose prefiltered levels are known
exactly: a one-texel checkerboard of two colours of equal luminance and exactly representable mean m is the constant m from level 1
on, so the GPU rendering the checkerboard with the bit follows the oracle rendering the constant-m map on the same random stream -
but only where every lookup the Metal kernel prefilters reads level >= 1 and every other lookup is absent.
"""
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(ROOT, "scenes")

pytestmark = pytest.mark.gpu

ENV_LOD = pt.PTR_METAL_ENV_LOD
SPEC = pt.PTR_METAL_SPECULAR
SSS = pt.PTR_METAL_SSS   # selects the Metal instantiation and changes nothing in scenes without subsurface materials
PBR = pt.PTR_METAL_PBR


def _write_env(path, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    pt.write_image(str(path), rgb, "pfm")
    assert np.array_equal(pt.read_pfm(str(path)), rgb)
    return str(path)


def _scene(tmp_path, text, name):
    p = tmp_path / name
    p.write_text(text)
    host = pt.HostScene.load(str(p), SCENES)
    return host


def _with(s, **kw):
    s = s.copy()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


SPHERE = """camera target=0,0,0 distance=4 yaw=0.3 pitch=0.2 vfov=30
renderer width=48 height=48 maxDepth=4 seed=1337 envRotation=0 envIntensity=1
background env={env}
material type=metal albedo=0.95,0.85,0.7 roughness={rough} name=m
sphere center=0,0,0 radius={radius} material=0
"""


# --------------------------------------------------------------------------- the lookup itself
def _restated_lookup(chain, dirs, rough, rotation, intensity):
    """numpy restatement in float32: envUv, environment_lod_from_roughness, bilinear per level with repeat addressing on both axes
    (texel centres at (i + 0.5) / W), linear between levels."""
    f = np.float32
    levels = len(chain)
    max_mip = f(levels - 1)
    a = np.clip(rough.astype(f), f(0), f(1))
    a = a * a
    lod = np.clip(a * max_mip, f(0), max_mip) if levels > 1 else np.zeros_like(a)
    d = dirs.astype(f)
    d = d / np.sqrt((d * d).sum(axis=1, dtype=f), dtype=f)[:, None].astype(f)
    c, s = f(np.cos(f(rotation))), f(np.sin(f(rotation)))
    rx, ry, rz = d[:, 0] * c - d[:, 2] * s, d[:, 1], d[:, 0] * s + d[:, 2] * c
    pi = f(np.pi)
    u = ((np.arctan2(rz, rx) + pi) / (f(2) * pi)).astype(f)
    v = (f(0.5) - np.arcsin(np.clip(ry, f(-1), f(1))) / pi).astype(f)

    def bilinear(level, idx):
        img = chain[level]
        H, W = img.shape[:2]
        fx, fy = u[idx] * f(W) - f(0.5), v[idx] * f(H) - f(0.5)
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = (x0 + 1) % W, (y0 + 1) % H
        x0, y0 = x0 % W, y0 % H
        ix, iy = f(1) - tx, f(1) - ty
        c00, c10, c01, c11 = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
        return (c00 * ix[:, None] + c10 * tx[:, None]) * iy[:, None] + (c01 * ix[:, None] + c11 * tx[:, None]) * ty[:, None]

    l0f = np.floor(lod)
    l0 = l0f.astype(np.int64)
    l1 = np.minimum(l0 + 1, levels - 1)
    frac = lod - l0f
    out = np.zeros((len(d), 4), f)
    for lv in range(levels):
        idx = np.nonzero(l0 == lv)[0]
        if len(idx):
            out[idx] = bilinear(lv, idx)
        idx = np.nonzero((l1 == lv) & (l1 != l0) & (frac > 0))[0]
        if len(idx):
            b = bilinear(lv, idx)
            out[idx] = out[idx] + (b - out[idx]) * frac[idx, None]
    return lod, out[:, :3] * f(max(intensity, 0.0))


def test_env_lookup_matches_restatement(tmp_path):
    rng = np.random.default_rng(7)
    w, h = 37, 19   # odd sizes: clamped second taps in the chain
    rgb = rng.uniform(0.5, 1.5, size=(h, w, 3)).astype(np.float32)
    env = _write_env(tmp_path / "odd.pfm", rgb)
    host = _scene(tmp_path, SPHERE.format(env=env, rough=0.5, radius=0.5), "odd.scene")
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for(width=16, height=16, environmentRotation=0.7, environmentIntensity=1.3)
    n = 50000
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    rough = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    rough[:4] = [0.0, 1.0, 0.5, 0.999]
    got = dev.env_lookup(s, np.concatenate([dirs, rough[:, None]], axis=1))
    rgba = np.concatenate([rgb, np.ones((h, w, 1), np.float32)], axis=2)
    chain = pt.debug_env_mips(rgba)
    assert len(chain) == 6
    lod, want = _restated_lookup(chain, dirs, rough, 0.7, 1.3)
    assert np.array_equal(got[:, 0], lod)                         # fp32 arithmetic, restated in fp32
    assert np.allclose(got[:, 1:], want, rtol=1e-5, atol=0)       # (ocml vs libm atan2 / asin)
    assert (lod > 1.0).mean() > 0.5 and (np.floor(lod) != lod).mean() > 0.9   # between levels, most of the time
    # a 1x1 map has no level beyond 0
    env1 = _write_env(tmp_path / "one.pfm", np.full((1, 1, 3), 0.25, np.float32))
    host1 = _scene(tmp_path, SPHERE.format(env=env1, rough=0.5, radius=0.5), "one.scene")
    got1 = pt.DeviceScene(host1.desc, 0, keepalive=host1).env_lookup(s, np.concatenate([dirs[:1000], rough[:1000, None]], axis=1))
    assert np.array_equal(got1[:, 0], np.zeros(1000, np.float32))
    assert np.allclose(got1[:, 1:], 0.25 * 1.3, rtol=1e-6)


# --------------------------------------------------------------------------- the lobe table
def test_sample_lobes_follow_the_metal_table():
    host = pt.HostScene.load(os.path.join(GOLDEN, "materials.scene"), SCENES)
    rng = np.random.default_rng(5)
    n = 2048
    wo = rng.normal(size=(n, 3))
    wo[:, 2] = np.abs(wo[:, 2]) + 0.1
    wo = (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(np.float32)
    inp = np.concatenate([rng.uniform(-1, 1, size=(n, 3)).astype(np.float32), np.tile(np.array([0, 0, 1], np.float32), (n, 1)), wo], axis=1)
    states = rng.integers(1, 2**32 - 1, size=n, dtype=np.uint64).astype(np.uint32)
    front = np.ones(n, dtype=np.uint32)
    mats = [host.desc.materials[i] for i in range(host.desc.materialCount)]
    base = mats[0]
    for t in range(8):   # every material type, whether or not the scene has one
        if not any(int(m.typeEta[0]) == t for m in mats):
            m = pt.PtrMaterial.from_buffer_copy(bytes(base))
            m.typeEta[0] = float(t)
            mats.append(m)
    for metallic, rough in ((0.0, 0.6), (1.0, 0.3), (0.5, 0.0)):   # the three metallic-roughness variants
        m = pt.PtrMaterial.from_buffer_copy(bytes(base))
        m.typeEta[0], m.typeEta[1], m.baseColorRoughness[3], m.pbrParams[0] = 7.0, 1.5, rough, metallic
        mats.append(m)
    seen = set()
    for sem in (0, SPEC, PBR):
        s = host.settings_for(width=16, height=16, metalSemantics=sem)
        for m in mats:
            t = int(m.typeEta[0])
            lobes, sample, st, env_rough = pt.debug_sample_lobes(m, s, inp, front, states)
            g, gs = pt.debug_sample_bsdf(m, s, inp, front, states)
            assert np.array_equal(sample.view(np.uint32), g.view(np.uint32)), (t, sem)   # the same samples, bit for bit
            assert np.array_equal(st, gs), (t, sem)
            assert np.array_equal(lobes[:, 2], g[:, 7])
            ok = g[:, 6] > 0
            lobe, lr = lobes[ok, 0], lobes[ok, 1]
            r = min(max(m.baseColorRoughness[3], 0.0), 1.0)
            coat_r = max(min(max(m.coatParams[0], 0.0), 1.0), 1e-3)
            if t == 0:
                assert (lobe == 0).all() and (lr == 1).all()
            elif t == 1:
                assert (lobe == 1).all() and np.allclose(lr, r)
            elif t == 2:
                assert (lobe == 1).all() and (lr == 0).all() and (lobes[ok, 2] == 1).all()
            elif t == 4:   # coat (1, coat roughness) or diffuse (0, 1)
                assert np.all(((lobe == 1) & np.isclose(lr, coat_r)) | ((lobe == 0) & (lr == 1)))
            elif t == 5 or t == 3:
                assert (lobe == 0).all() and (lr == 0).all()
            elif t == 6:   # coat, flake, base specular at their roughness; base diffuse (0, 1)
                flake_r = max(min(max(m.carpaintFlakeParams[1], 0.0), 1.0), 1e-3)
                base_r = max(min(max(m.carpaintBaseParams[1], 0.0), 1.0), 1e-3)
                spec = (lobe == 1) & (np.isclose(lr, coat_r) | np.isclose(lr, flake_r) | np.isclose(lr, base_r))
                assert np.all(spec | ((lobe == 0) & (lr == 1)))
            elif t == 7:   # specular (1, r), diffuse (0, 1), transmission (2, r: Metal model only)
                assert np.all(((lobe == 1) & np.isclose(lr, r)) | ((lobe == 0) & (lr == 1)) | ((lobe == 2) & np.isclose(lr, r)))
                assert sem == PBR or not (lobe == 2).any()
            seen.update((t, int(x)) for x in np.unique(lobe))
            want_env = {1: r, 7: r, 4: coat_r, 6: min(max(m.carpaintBaseParams[1], 0.0), 1.0)}.get(t, 1.0)
            assert np.isclose(env_rough, want_env, rtol=1e-6), t
    assert {(1, 1), (2, 1), (4, 1), (4, 0), (6, 1), (6, 0), (7, 1), (7, 0), (0, 0)} <= seen


# --------------------------------------------------------------------------- same random stream as the oracle
C1 = np.array([0.6, 0.5, 0.5 - 0.1 * 0.2126 / 0.0722], np.float32)   # c1 - m is orthogonal to the luminance weights
M = np.array([0.5, 0.5, 0.5], np.float32)
C2 = (np.float32(1.0) - C1).astype(np.float32)                     # exact: c1 + c2 = 2 m, so every level >= 1 of the board is m


def _board(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx + yy) % 2 == 0)[..., None], C1, C2).astype(np.float32)


def _stream_parity(dev, s_gpu, osc, s_ref, high_spp):
    img1, st1 = dev.render_image(s_gpu, 1, count=True)
    ref1, _, c1 = osc.render(s_ref, 1, threads=0, count=True)
    frac = float((np.abs(img1 - ref1) / (np.abs(ref1) + 1e-2)).max(axis=2).__le__(1e-3).mean())
    counters = (abs(st1.extendRays - c1["extendRays"]) <= 0.002 * c1["extendRays"] + 2 and
                abs(st1.shadedHits - c1["shadedHits"]) <= 0.002 * c1["shadedHits"] + 2)
    imgN, _ = dev.render_image(s_gpu, high_spp)
    refN, _, _ = osc.render(s_ref, high_spp, threads=0)
    refM, _, _ = osc.render(_with(s_ref, seed=1338), high_spp, threads=0)
    lum = np.array([0.2126, 0.7152, 0.0722])
    return frac, counters, _rmse(imgN, refN), _rmse(refN, refM), float((imgN @ lum).mean() / (refN @ lum).mean())


@pytest.mark.parametrize("model", ["metal", "pbr"])
def test_checkerboard_follows_the_oracle_on_the_constant_mean(tmp_path, model):
    w, h = 64, 32
    board = _write_env(tmp_path / "board.pfm", _board(w, h))
    mean = _write_env(tmp_path / "mean.pfm", np.broadcast_to(M, (h, w, 3)))
    rgba = np.concatenate([_board(w, h), np.ones((h, w, 1), np.float32)], axis=2)
    chain = pt.debug_env_mips(rgba)
    assert len(chain) == 7 and all(np.array_equal(lv[..., :3], np.broadcast_to(M, lv[..., :3].shape)) for lv in chain[1:])
    # equal luminance: the importance tables of the board and of the constant map agree to a few ulps
    db = pt.debug_env_distribution(rgba)
    dm = pt.debug_env_distribution(np.concatenate([np.broadcast_to(M, (h, w, 3)), np.ones((h, w, 1))], axis=2).astype(np.float32))
    assert np.allclose(db["pdf"], dm["pdf"], rtol=1e-5) and np.allclose(db["marg_threshold"], dm["marg_threshold"], atol=1e-5)
    hb = _scene(tmp_path, SPHERE.format(env=board, rough=0.5, radius=1.8), "board.scene")
    hm = _scene(tmp_path, SPHERE.format(env=mean, rough=0.5, radius=1.8), "mean.scene")
    if model == "pbr":   # metallic 1, roughness 0.5: the diffuse lobe has no weight, so no path reads level 0 after it
        for hs in (hb, hm):
            mat = hs.desc.materials[0]
            mat.typeEta[0], mat.typeEta[1], mat.pbrParams[0] = 7.0, 1.5, 1.0
    sem = SPEC if model == "metal" else PBR
    dev, osc = pt.DeviceScene(hb.desc, 0, keepalive=hb), ol.OracleScene(hm)
    s = hb.settings_for(width=48, height=48, max_depth=4, seed=1337)
    albedo, _ = dev.render_aovs(s, 0)
    assert (albedo[..., 3] == 1.0).all()   # the sphere fills the frame: no camera ray misses
    # maxMip 6, roughness 0.5: every prefiltered lookup is at LOD 1.5 and returns m
    frac, counters, err, noise, ratio = _stream_parity(dev, _with(s, metalSemantics=sem | ENV_LOD), osc, _with(s, metalSemantics=sem), 32)
    assert counters
    assert frac >= 0.99, frac   # measured: 1.0 for both models
    assert err <= 1.25 * noise, (err, noise)
    assert abs(ratio - 1.0) <= 0.005, ratio
    # without the bit every lookup reads the board at level 0
    frac0, _, _, _, _ = _stream_parity(dev, _with(s, metalSemantics=sem), osc, _with(s, metalSemantics=sem), 4)
    assert frac0 < 0.5, frac0


# --------------------------------------------------------------------------- where the bit must change nothing
NO_LOD = """camera target=0,0.5,0 distance=6 yaw=0.4 pitch=0.15 vfov=40
renderer width=64 height=48 maxDepth=6 seed=1337 envRotation=20 envIntensity=1
background env=assets/sky_96x48.hdr
material type=lambert albedo=0.7,0.6,0.5 name=l
material type=metal albedo=0.9,0.9,0.9 roughness=0.0 name=mirror
material type=dielectric ior=1.5 name=glass
sphere center=-1.3,0.5,0 radius=0.6 material=0
sphere center=0,0.5,0 radius=0.6 material=1
sphere center=1.3,0.5,0 radius=0.6 material=2
sphere center=0,-100,0 radius=99.9 material=0
"""


def _env_materials_with(tmp_path, env, name):
    text = open(os.path.join(GOLDEN, "env_materials.scene")).read().replace("background env=assets/sky_96x48.hdr", "background env=" + env)
    assert ("background env=" + env) in text
    return _scene(tmp_path, text, name)


def test_no_prefiltered_lookup_means_the_same_image(tmp_path):
    from scenes.gen_assets import ensure_assets

    ensure_assets()
    # Lambert (environment-lighting roughness 1, diffuse lobe), mirror and glass (delta): no lookup qualifies
    host = _scene(tmp_path, NO_LOD, "no_lod.scene")
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for(width=64, height=48, max_depth=6, seed=1337)
    off, _ = dev.render_image(_with(s, metalSemantics=SPEC | SSS), 8)
    on, _ = dev.render_image(_with(s, metalSemantics=SPEC | SSS | ENV_LOD), 8)
    assert off.mean() > 0.01 and np.array_equal(on, off)
    # rough metal, plastic and car paint under a 1x1 map: maxMip 0, nothing to prefilter
    one = _write_env(tmp_path / "one.pfm", np.array([[[0.8, 0.6, 0.4]]], np.float32))
    host = _env_materials_with(tmp_path, one, "env1.scene")
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for(width=64, height=48, max_depth=6, seed=1337)
    off, _ = dev.render_image(_with(s, metalSemantics=SPEC | SSS), 8)
    on, _ = dev.render_image(_with(s, metalSemantics=SPEC | SSS | ENV_LOD), 8)
    assert off.mean() > 0.01 and np.array_equal(on, off)


def test_constant_map_prefiltered_equals_level_zero(tmp_path):
    # every level of a constant map is the constant: a missing intensity / rotation or a wrong level offset would show
    const = _write_env(tmp_path / "const.pfm", np.broadcast_to(np.array([0.7, 0.5, 0.3], np.float32), (16, 32, 3)))
    host = _env_materials_with(tmp_path, const, "const.scene")
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for(width=64, height=48, max_depth=6, seed=1337, environmentIntensity=1.7, environmentRotation=0.9)
    off, _ = dev.render_image(_with(s, metalSemantics=SPEC | SSS), 8)
    on, _ = dev.render_image(_with(s, metalSemantics=SPEC | SSS | ENV_LOD), 8)
    assert off.mean() > 0.01
    assert np.allclose(on, off, rtol=1e-5, atol=1e-6), float(np.abs(on - off).max())


def test_no_stale_state_and_scheduling_invariance(tmp_path):
    board = _write_env(tmp_path / "board.pfm", _board(64, 32))
    host = _scene(tmp_path, SPHERE.format(env=board, rough=0.5, radius=0.7), "open.scene")
    s = host.settings_for(width=512, height=512, max_depth=4, seed=1337)
    on_s, off_s = _with(s, metalSemantics=SPEC | SSS | ENV_LOD), _with(s, metalSemantics=SPEC | SSS)

    def render(env, settings):
        os.environ.update(env)       # the knobs are read when the scene is uploaded
        try:
            dev = pt.DeviceScene(host.desc, 0, keepalive=host)
            image, _ = dev.render_image(settings, 16)
            albedo, _ = dev.render_aovs(settings, 0)
            dev.close()
        finally:
            for k in env:
                del os.environ[k]
        return image, albedo

    on, albedo = render({}, on_s)
    off, _ = render({}, off_s)
    # pixels whose camera rays all miss (two pixels away from the silhouette of sample 0): background at level 0 either way
    hit = albedo[..., 3] > 0
    near = hit.copy()
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            near |= np.roll(np.roll(hit, dy, axis=0), dx, axis=1)
    miss = ~near
    assert 0.2 < hit.mean() < 0.8 and miss.mean() > 0.2
    assert np.array_equal(on[miss], off[miss])
    assert not np.allclose(on[hit], off[hit])   # and the sphere's reflections do change
    # 4 Mi work items, 2 Mi slots: the scheduling knobs of the invariance test must not show either
    for env in ({"PTR_POOL_GROUPS": "1"}, {"PTR_POOL_GROUPS": "4"}, {"PTR_CONNECT_OVERLAP": "0"}, {"PTR_TAIL_BELOW": "0"},
                {"PTR_POOL_SLOTS": str(3 << 18), "PTR_REFILL_BELOW": "24"}, {"PTR_MAX_ITEMS": str(512 * 512 * 16)}):
        image, _ = render(env, on_s)
        assert np.array_equal(image, on), env


# --------------------------------------------------------------------------- routing and CLI
def test_routing_and_cli(tmp_path):
    from scenes.gen_assets import ensure_assets

    ensure_assets()
    host = pt.HostScene.load(os.path.join(GOLDEN, "env_materials.scene"), SCENES)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for(width=64, height=48, max_depth=6, seed=1337)
    assert dev.shade_kernel_set(_with(s, metalSemantics=ENV_LOD)) == 0x3FF
    assert dev.shade_kernel_set(_with(s, metalSemantics=SPEC | ENV_LOD)) == 0x3FF
    out = tmp_path / "frame.pfm"
    r = subprocess.run([pt.CLI_PATH, "--scene=" + os.path.join(GOLDEN, "env_materials.scene"), "--assets=" + SCENES, "--width=64", "--height=48",
                        "--sppTotal=4", "--seed=1337", "--format=pfm", "--output=" + str(out), "--devices=1", "--semantics=metal-envlod"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img, _ = dev.render_image(_with(s, metalSemantics=255), 4)
    assert np.array_equal(pt.read_pfm(str(out)), img)
    img127, _ = dev.render_image(_with(s, metalSemantics=127), 4)
    assert not np.array_equal(img127, img)
