"""GPU tests of the first-hit feature buffers (k_aovs and k_surface, csrc/kernels/wavefront.hip reportedSurface) against the rule stated at
ptr_render_aovs in include/ptr_abi.h, pixel by pixel.

Rule 1 is held to tests/aov_ref.py, a float64 statement on the oracle's hits: hit mask, distance and albedo bit for bit, the normal within
max(8 x the float32 twin's largest difference from float64 over the case, 2^-22).  Pixels where ptr_trace_rays names another primitive
than the oracle (a ray on an edge two triangles share) are left out, and may be 0.1 % of a case's hit pixels, the share
tests/test_gpu_traversal.py allows.  Rules 2 and 3 are held, bit for bit, to the probes that run applyPbrTextures on rows of their own
(ptr_debug_first_hit_textures, ptr_debug_pbr_hits) along the vertices ptr_debug_path_states records of the production loop; those probes
are held to float64 by tests/test_gpu_ray_diff.py and tests/test_gpu_pbr_hit.py.  Rule 4 is held to ptr_render_aovs through a temporal step.
"""
import os

import numpy as np
import pytest
import torch

import aov_ref as A
import oracle_lib as ol
import pbr_hit_domain as D
import test_gpu_traversal as T

pt = ol.pt
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ol.ROOT, "tests", "golden")
SCENES = os.path.join(ol.ROOT, "scenes")
F = np.float32
PBR, RAY_DIFF, FACE_NORMAL = pt.PTR_METAL_PBR, pt.PTR_METAL_RAY_DIFF, pt.PTR_METAL_FACE_NORMAL
TIE_SHARE = 0.001
SIZES = ((1, 1), (37, 21), (96, 64))
SAMPLES = (0, 3)
DEFOCUS = (0.0, 1.5)


# --------------------------------------------------------------------------------------------------------------------- scenes
CAMERA = "camera target=0,0,0 distance=6 yaw=1.2 pitch=0.45 vfov=40\nrenderer width=96 height=64 maxDepth=6 seed=1337\nbackground solid=0.2,0.3,0.4\n"


def _load_text(tmp, name, text):
    path = os.path.join(str(tmp), name + ".scene")
    with open(path, "w") as f:
        f.write(text)
    return pt.HostScene.load(path, SCENES)


def _plain_material(kind, base):
    m = pt.PtrMaterial()
    m.baseColorRoughness[:] = [base[0], base[1], base[2], 0.5]
    m.typeEta[:] = [float(kind), 1.5, 1.5, 0.0]
    m.textureIndices0[:] = [0xFFFFFFFF] * 4
    m.textureIndices1[:] = [0xFFFFFFFF] * 4
    return m


def _materials_host():
    """tests/golden/materials.scene (seven material types on spheres over a rectangle) with the two types its grammar cannot name put in:
    the mirror becomes an emitter, the floor a metallic-roughness material; and one base colour leaves [0, 1]."""
    host = pt.HostScene.load(os.path.join(GOLDEN, "materials.scene"), SCENES)
    m = host.desc.materials
    m[2].typeEta[0] = 3.0
    m[2].emission[:] = [2.0, 2.0, 2.0, 0.0]
    m[10].typeEta[0] = 7.0
    m[1].baseColorRoughness[:] = [1.5, -0.25, 0.5, 0.35]
    assert {int(m[i].typeEta[0]) for i in range(host.desc.materialCount)} == set(range(8))
    return host


def _normals_mesh(material=0):
    """A field of separate triangles on y = 0 whose vertex normals are, by column of the field: tilted to the geometric side, tilted to
    the other side, zero at every vertex, and zero at one vertex."""
    rng = np.random.default_rng(11)
    pos, nrm, idx = [], [], []
    for i in range(12):
        for j in range(12):
            x, z = -3.0 + 0.5 * i, -3.0 + 0.5 * j
            base = len(pos)
            pos += [[x, 0.0, z], [x, 0.0, z + 0.48], [x + 0.48, 0.0, z]]      # cross(e1, e2) points to +y
            tilt = [np.array([rng.uniform(-0.6, 0.6), 1.0, rng.uniform(-0.6, 0.6)]) * rng.uniform(0.5, 2.0) for _ in range(3)]
            kind = i % 4
            if kind == 1:
                tilt = [-t for t in tilt]
            elif kind == 2:
                tilt = [np.zeros(3)] * 3
            elif kind == 3:
                tilt[j % 3] = np.zeros(3)
            nrm += [list(t) for t in tilt]
            idx.append([base, base + 1, base + 2])
    return {"positions": np.array(pos), "normals": np.array(nrm), "indices": np.array(idx), "material": material}


def _box_mesh(half, material):
    """A closed box about the origin, outward winding, with corner normals that are not the faces' (a dielectric must not use them)."""
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = []
    for q in quads:
        a, b, cc, d = q
        n = np.cross(c[b] - c[a], c[cc] - c[a])
        centre = c[list(q)].mean(axis=0)
        tris = [[a, b, cc], [a, cc, d]] if np.dot(n, centre) > 0 else [[a, cc, b], [a, d, cc]]
        idx += tris
    return {"positions": c * half, "normals": c / np.sqrt(3.0), "indices": np.array(idx), "material": material}


class _Host:
    """what the cases need of a host scene, for a description made in Python (pbr_hit_domain.Scene)"""

    def __init__(self, scene, settings_host):
        self.scene, self.desc, self._settings = scene, scene.desc, settings_host

    def settings_for(self, **kw):
        return self._settings.settings_for(**kw)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """name -> (host, metalSemantics values the case runs under); built once, with one device scene and one oracle scene each"""
    tmp = tmp_path_factory.mktemp("aovs")
    camera_only = _load_text(tmp, "camera", CAMERA + "material type=lambert albedo=0.5,0.5,0.5\n")
    glass, grey = _plain_material(2, (0.9, 0.95, 1.0)), _plain_material(0, (0.3, 0.6, 0.2))
    table = {
        "materials": (_materials_host(), (0, FACE_NORMAL)),
        "mesh-normals": (_Host(D.Scene([_normals_mesh()], [grey], []), camera_only), (0,)),
        "inside-dielectric-mesh": (_Host(D.Scene([_box_mesh(20.0, 0), _normals_mesh(1)], [glass, grey], []), camera_only), (0, FACE_NORMAL)),
        "inside-dielectric-sphere": (_load_text(tmp, "sphere", CAMERA + "material type=dielectric ior=1.5\nmaterial type=lambert albedo=0.7,0.2,0.1\n"
                                                "sphere center=0,0,0 radius=20 material=0\nsphere center=0,0,0 radius=1 material=1\n"), (0, FACE_NORMAL)),
        "textured-without-pbr": (pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN), (0,)),
        "empty": (camera_only, (0,)),
        "no-materials": (_Host(D.Scene([_normals_mesh()], [], []), camera_only), (0,)),
    }
    built = {}
    for name, (host, semantics) in table.items():
        built[name] = (host, pt.DeviceScene(host.desc, 0, keepalive=host), ol.OracleScene(host), semantics)
    return built


# --------------------------------------------------------------------------------------------------------------------- rule 1
def _xys(s, sample):
    ys, xs = np.meshgrid(np.arange(s.height, dtype=np.uint32), np.arange(s.width, dtype=np.uint32), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), np.full(s.width * s.height, sample, np.uint32)], axis=1)


def _batch(rays):
    n = len(rays)
    return np.concatenate([rays[:, :3], np.full((n, 1), 1e-4, F), rays[:, 3:6], np.full((n, 1), np.inf, F)], axis=1).astype(F)


def _same_primitive(a, b):
    return (a["primType"] == b["primType"]) & (a["geomIndex"] == b["geomIndex"]) & (a["primIndex"] == b["primIndex"])


def _rule1_rows(desc, dev, osc, rays, semantics, where):
    """Rule 1 at the closest hits of rays [n, 6]: (float64 reference, tolerance of the normal, mask of the rows that are no ties)."""
    batch = _batch(rays)
    hits = osc.trace_rays(batch, any_hit=False)
    surface = osc.surface_hits(np.concatenate([rays[:, :6], rays[:, 3:6]], axis=1))
    ref64 = A.first_hit_features(desc, hits, surface, semantics, np.float64)
    ref32 = A.first_hit_features(desc, hits, surface, semantics, np.float32)
    mine = dev.trace_rays(batch)[0]
    assert np.array_equal(mine["t"] >= 0, hits["t"] >= 0), where
    hit = hits["t"] >= 0
    tie = hit & ~_same_primitive(mine, hits)
    assert tie.sum() <= TIE_SHARE * max(int(hit.sum()), 1), (where, "ties", int(tie.sum()), int(hit.sum()), np.flatnonzero(tie)[:8])
    return ref64, A.normal_tolerance(ref64, ref32), ~tie


def _first_bad(mask, width):
    at = np.flatnonzero(mask)[:6]
    return [(int(i % width), int(i // width)) for i in at]


def _check_rule1(got_albedo, got_normal, ref, tol, use, where, width):
    """got_*: [n, 4] rows of the two buffers; ref: aov_ref rows; use: the rows to hold"""
    hit = ref["hit"]
    bad = use & ((got_albedo[:, 3] > 0.5) != hit)
    assert not bad.any(), (where, "hit mask", _first_bad(bad, width))
    assert set(np.unique(got_albedo[:, 3])) <= {0.0, 1.0}, where
    bad = use & (got_normal[:, 3].view(np.uint32) != ref["distance"].view(np.uint32))
    assert not bad.any(), (where, "distance", _first_bad(bad, width))
    bad = use & (got_albedo[:, :3].view(np.uint32) != ref["albedo"].view(np.uint32)).any(axis=1)
    assert not bad.any(), (where, "albedo", _first_bad(bad, width), got_albedo[bad][:3], ref["albedo"][bad][:3])
    miss = use & ~hit
    assert (got_albedo[miss] == 0).all() and (got_normal[miss, :3] == 0.5).all() and (got_normal[miss, 3] == 0).all(), (where, "miss pixels")
    err = np.abs(got_normal[:, :3].astype(np.float64) - ref["normal"]).max(axis=1)
    worst = float(err[use & hit].max()) if (use & hit).any() else 0.0
    bad = use & hit & (err > tol)
    assert not bad.any(), (where, "normal", worst, tol, _first_bad(bad, width))
    return worst


CASES = ["materials", "mesh-normals", "inside-dielectric-mesh", "inside-dielectric-sphere", "textured-without-pbr", "empty", "no-materials"]


@pytest.mark.parametrize("name", CASES)
def test_rule_1_every_pixel_against_float64(cases, name):
    host, dev, osc, semantics_of = cases[name]
    seen = {"hit": 0, "back-glass": 0, "fallback": 0, "opposed": 0}
    for semantics in semantics_of:
        for width, height in SIZES:
            for sample in SAMPLES:
                for defocus in DEFOCUS:
                    s = host.settings_for(width=width, height=height, max_depth=4, seed=1337, cameraDefocusAngle=defocus, cameraFocusDistance=6.0)
                    s.metalSemantics = semantics
                    where = "%s, semantics %d, %dx%d, sample %d, defocus %g" % (name, semantics, width, height, sample, defocus)
                    rays, _ = ol.camera_rays(s, _xys(s, sample))
                    mine, _ = pt.debug_camera_rays(s, _xys(s, sample))
                    assert np.array_equal(rays, mine), where
                    ref, tol, use = _rule1_rows(host.desc, dev, osc, rays, semantics, where)
                    albedo, normal = dev.render_aovs(s, sample)
                    worst = _check_rule1(albedo.reshape(-1, 4), normal.reshape(-1, 4), ref, tol, use, where, width)
                    if (width, height) == SIZES[-1]:
                        print("%s: hit %d of %d, ties %d, normal: largest difference %.3g, bound %.3g" % (where, ref["hit"].sum(), len(rays), (~use).sum(), worst, tol))
                    seen["hit"] += int(ref["hit"].sum())
    # the case is what it is named for
    s = host.settings_for(width=96, height=64, max_depth=4, seed=1337, cameraDefocusAngle=0.0)
    rays, _ = ol.camera_rays(s, _xys(s, 0))
    hits = osc.trace_rays(_batch(rays), any_hit=False)
    surface = osc.surface_hits(np.concatenate([rays, rays[:, 3:6]], axis=1))
    hit = hits["t"] >= 0
    if name in ("empty", "no-materials"):
        albedo, normal = dev.render_aovs(s, 0)
        assert (albedo == 0).all() and (normal[..., :3] == 0.5).all() and (normal[..., 3] == 0).all()
        assert hit.any() == (name == "no-materials")
        return
    assert seen["hit"] > 1000
    material = A.hit_materials(host.desc, hits)
    _, types = A.material_table(host.desc)
    glass_back = hit & (types[material] == 2) & (surface[:, 11] == 0)
    if name == "materials":
        assert set(np.unique(types[material[hit]])) == set(range(8))
    if name.startswith("inside-dielectric"):
        assert glass_back.sum() > 500
    if name == "inside-dielectric-mesh":   # the corner normals are not the faces': the dielectric rule shows
        cos = (surface[glass_back, 5:8] * surface[glass_back, 8:11]).sum(axis=1)
        assert (np.abs(cos) < 0.999).sum() > 300
    if name == "mesh-normals":
        # opposed vertex normals are turned to the ray's side by the hit record; zero ones fall back to the geometric normal
        geometric_up = np.abs(np.abs(surface[hit, 8:11]) - np.abs(surface[hit, 5:8])).max(axis=1) == 0
        assert geometric_up.sum() > 200 and (~geometric_up).sum() > 400


# --------------------------------------------------------------------------------------------------------------------- rules 2 and 3
@pytest.fixture(scope="module")
def textured(cases):
    host, dev, osc, _ = cases["textured-without-pbr"]
    return host, dev, osc


def _textured_settings(host, semantics, **kw):
    s = host.settings_for(width=kw.pop("width", 96), height=kw.pop("height", 72), max_depth=kw.pop("max_depth", 6), seed=1337, cameraDefocusAngle=0.0)
    s.metalSemantics = semantics
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _encode(n):
    return (n.astype(F) * F(0.5) + F(0.5)).astype(F)


def _clamped(c):
    return np.clip(c.astype(F), F(0.0), F(1.0))


def _walk(host, dev, osc, s, sample):
    """The surface rule 3 reports for every pixel of sample `sample`, from the probes: vertex 0 by ptr_debug_first_hit_textures, every
    later vertex by ptr_debug_pbr_hits on the ray, cone and random state ptr_debug_path_states recorded after the vertex before.
    Returns a dict of per-pixel arrays: albedo [n, 3] and normal [n, 3] (encoded) exact where `exact`, else rule 1 (`ref`, `tol`, `use`);
    distance, hit, passes (surfaces passed through), and the first vertex's facts."""
    n = s.width * s.height
    xys = _xys(s, sample)
    rays, states = pt.debug_camera_rays(s, xys)
    first = dev.first_hit_textures(s, xys)
    ref0, tol0, use0 = _rule1_rows(host.desc, dev, osc, rays, s.metalSemantics, "vertex 0")
    out = {"albedo": ref0["albedo"].copy(), "normal": ref0["normal"].copy(), "distance": ref0["distance"].copy(), "hit": ref0["hit"].copy(),
           "exact": np.zeros(n, bool), "use": use0.copy(), "tol": tol0, "passes": np.zeros(n, np.int64),
           "first_textured": first["textured"] > 0, "first_discard": first["discard"] > 0, "first": first, "camera_states": states, "rays": rays}
    kept = (first["textured"] > 0) & ~(first["discard"] > 0)
    assert np.array_equal(first["t"][first["textured"] > 0], ref0["distance"][first["textured"] > 0])
    out["albedo"][kept] = _clamped(first["base_color"][kept])
    out["normal"][kept] = _encode(first["normal"][kept])
    out["exact"][kept] = True
    active = np.flatnonzero(first["discard"] > 0)
    snap, ran, _ = dev.path_states(s, np.arange(n, dtype=np.uint32), sample, s.maxDepth + 1)
    # the production loop saw the same first vertex
    on = first["textured"] > 0
    assert np.array_equal(snap["t"][0][on], first["t"][on])
    out["later_rows"], out["later_got"] = [], []
    total = first["t"].astype(F).copy()
    for k in range(1, s.maxDepth + 1):
        if len(active) == 0:
            break
        out["passes"][active] = k
        if k >= s.maxDepth:          # the path ended on a surface it passed through
            out["hit"][active], out["albedo"][active], out["normal"][active], out["distance"][active] = False, 0.0, 0.5, 0.0
            out["exact"][active] = True
            break
        assert ran > k
        origin, direction = snap["origin"][k - 1][active], snap["direction"][k - 1][active]
        assert np.array_equal(direction, rays[active, 3:6]), "a pass-through keeps the direction"
        cone = snap["cone"][k - 1][active]
        assert (cone == cone[0]).all(), "a pass-through keeps the primary cone"
        rows = pt.DeviceScene.pbr_hit_rows(np.concatenate([origin, direction], axis=1), cone, snap["rng"][k - 1][active])
        got = dev.pbr_hits(rows)
        out["later_rows"].append(rows)
        out["later_got"].append(got)
        here = got["hit"] > 0
        assert np.array_equal(got["t"][here], snap["t"][k][active][here]), "the probe and the production loop trace the same segment"
        total[active] = (total[active] + np.where(here, got["t"], F(0.0)).astype(F)).astype(F)
        # the misses
        gone = active[~here]
        out["hit"][gone], out["albedo"][gone], out["normal"][gone], out["distance"][gone], out["exact"][gone] = False, 0.0, 0.5, 0.0, True
        # textured and kept: the probe's own values
        tex = here & (got["textured"] > 0)
        keep = tex & ~(got["discard"] > 0)
        at = active[keep]
        out["albedo"][at], out["normal"][at] = _clamped(got["base_color"][keep]), _encode(got["normal"][keep])
        out["hit"][at], out["distance"][at], out["exact"][at] = True, total[at], True
        # another kind of surface: rule 1 on this segment
        plain = here & ~tex
        if plain.any():
            ref, tol, use = _rule1_rows(host.desc, dev, osc, np.concatenate([origin, direction], axis=1)[plain], s.metalSemantics, "vertex %d" % k)
            at = active[plain]
            out["albedo"][at], out["normal"][at], out["hit"][at], out["distance"][at] = ref["albedo"], ref["normal"], True, total[at]
            out["use"][at] = use
            out["tol"] = max(out["tol"], tol)
        again = tex & (got["discard"] > 0)
        if k + 1 < s.maxDepth:   # (a path that ends at this vertex keeps no state)
            assert np.array_equal(got["state"][again], snap["rng"][k][active][again]), "the random state after a discard is the path's"
        active = active[again]
    return out


def _check_walk(w, albedo, normal, where, width):
    a, nrm = albedo.reshape(-1, 4), normal.reshape(-1, 4)
    ref = {"hit": w["hit"], "albedo": w["albedo"], "normal": w["normal"], "distance": w["distance"]}
    _check_rule1(a, nrm, ref, w["tol"], w["use"] & ~w["exact"], where, width)
    ex = w["exact"]
    bad = ex & ((a[:, 3] > 0.5) != w["hit"])
    assert not bad.any(), (where, "hit mask", _first_bad(bad, width))
    bad = ex & (a[:, :3].view(np.uint32) != w["albedo"].view(np.uint32)).any(axis=1)
    assert not bad.any(), (where, "albedo", _first_bad(bad, width), a[bad][:3], w["albedo"][bad][:3])
    bad = ex & (nrm[:, :3].view(np.uint32) != w["normal"].astype(F).view(np.uint32)).any(axis=1)
    assert not bad.any(), (where, "normal", _first_bad(bad, width), nrm[bad][:3], w["normal"][bad][:3])
    bad = ex & (nrm[:, 3].view(np.uint32) != w["distance"].view(np.uint32))
    assert not bad.any(), (where, "distance", _first_bad(bad, width), nrm[bad][:3, 3], w["distance"][bad][:3])


@pytest.fixture(scope="module")
def walks(textured):
    host, dev, osc = textured
    cache = {}

    def get(semantics, sample):
        if (semantics, sample) not in cache:
            s = _textured_settings(host, semantics)
            cache[(semantics, sample)] = (s, _walk(host, dev, osc, s, sample), dev.render_aovs(s, sample))
        return cache[(semantics, sample)]

    return get


@pytest.mark.parametrize("semantics", [PBR, PBR | RAY_DIFF])
def test_rule_2_textured_first_hits(textured, walks, semantics):
    host, dev, osc = textured
    for sample in SAMPLES:
        s, w, (albedo, normal) = walks(semantics, sample)
        where = "textured, semantics %d, sample %d" % (semantics, sample)
        first = w["first"]
        kept = w["first_textured"] & ~w["first_discard"]
        a, nrm = albedo.reshape(-1, 4), normal.reshape(-1, 4)
        assert np.array_equal(a[kept, :3], _clamped(first["base_color"][kept])), where
        assert np.array_equal(nrm[kept, :3], _encode(first["normal"][kept])), where
        assert np.array_equal(nrm[kept, 3], first["t"][kept]) and (a[kept, 3] == 1).all(), where
        plain = ~w["first_textured"]
        ref = {k: w[k] for k in ("hit", "albedo", "normal", "distance")}
        _check_rule1(a, nrm, ref, w["tol"], plain & w["use"], where, s.width)
        # what rule 1 alone would say at the kept textured hits: the factor and the interpolated normal
        rule1 = A.first_hit_features(host.desc, osc.trace_rays(_batch(w["rays"]), any_hit=False),
                                     osc.surface_hits(np.concatenate([w["rays"], w["rays"][:, 3:6]], axis=1)), semantics)
        mapped = kept & w["use"] & (np.abs(nrm[:, :3] - rule1["normal"]).max(axis=1) > 1e-3)
        coloured = kept & w["use"] & (np.abs(a[:, :3] - rule1["albedo"]).max(axis=1) > 1e-3)
        print("%s: textured kept %d, normal differs from the interpolated one at %d, albedo from the factor at %d" % (where, kept.sum(), mapped.sum(), coloured.sum()))
        assert kept.sum() > 3000 and mapped.sum() > 300 and coloured.sum() > 1000, where
    if semantics & RAY_DIFF:   # the gradients reach the buffers: some first hit is textured differently than by the cone
        other = walks(PBR, 0)[2]
        assert not np.array_equal(other[0], walks(semantics, 0)[2][0])


@pytest.mark.parametrize("semantics", [PBR, PBR | RAY_DIFF])
def test_rule_3_discarded_hits_are_passed_through(textured, walks, semantics):
    host, dev, osc = textured
    modes = np.array([host.desc.materials[i].pbrExtras[3] for i in range(host.desc.materialCount)])
    discards = {}
    for sample in SAMPLES:
        s, w, (albedo, normal) = walks(semantics, sample)
        where = "textured, semantics %d, sample %d" % (semantics, sample)
        _check_walk(w, albedo, normal, where, s.width)
        hits0 = osc.trace_rays(_batch(w["rays"]), any_hit=False)
        mode = modes[A.hit_materials(host.desc, hits0)]
        mask, blend = w["first_discard"] & (mode == 1), w["first_discard"] & (mode == 2)
        discards[sample] = (w["first_discard"], w["first_textured"] & (mode == 2))
        print("%s: discards MASK %d BLEND %d, passes %s, pixels left without a surface %d"
              % (where, mask.sum(), blend.sum(), np.bincount(w["passes"]).tolist(), (w["first_discard"] & ~w["hit"]).sum()))
        assert mask.sum() >= 20 and blend.sum() >= 20 and (w["passes"] >= 2).sum() >= 1, where
        moved = w["first_discard"] & w["hit"]
        assert (normal.reshape(-1, 4)[moved, 3] > w["first"]["t"][moved]).all(), where
        # the oracle's applyPbrTextures on the same rows (it has no gradient path: the later vertices, and vertex 0 without RAY_DIFF)
        rows = list(w["later_rows"])
        got = list(w["later_got"])
        if not (semantics & RAY_DIFF):
            on = w["first_textured"]
            cone0 = np.broadcast_to(w["later_rows"][0][0, 6:8], (int(on.sum()), 2)) if rows else np.zeros((int(on.sum()), 2), F)
            rows.append(pt.DeviceScene.pbr_hit_rows(w["rays"][on], cone0, w["camera_states"][on]))
            got.append(dev.pbr_hits(rows[-1]))
            assert np.array_equal(got[-1]["discard"] > 0, w["first_discard"][on]), "the two probes of vertex 0 agree"
        for r, g in zip(rows, got):
            o = osc.pbr_hits(r)
            same = (g["hit"] > 0) & (o["hit"] > 0) & (g["mesh"] == o["mesh"]) & (g["triangle"] == o["triangle"])
            assert same.sum() >= 0.99 * max(int((g["hit"] > 0).sum()), 1), where
            assert np.array_equal(g["textured"][same], o["textured"][same]), where
            # the decisions and states: equal but for a row on a threshold (tests/test_gpu_pbr_hit.py allows 2 % of the textured rows)
            differ = same & ((g["discard"] != o["discard"]) | (g["state"] != o["state"]))
            assert differ.sum() <= 0.02 * max(int((g["textured"] > 0).sum()), 1), (where, int(differ.sum()))
            both = same & ~differ & (g["textured"] > 0) & ~(g["discard"] > 0)
            if both.any():
                worst = float(np.abs(g["base_color"][both].astype(np.float64) - o["base_color"][both]).max())
                assert worst <= 8 * D.EPS32 * max(1.0, float(np.abs(o["base_color"][both]).max())), (where, worst)
    # at most maxDepth surfaces: at depth 1 every discarded first hit leaves a miss pixel, at depth 2 the pixels that pass two surfaces do
    if not (semantics & RAY_DIFF):
        for depth in (1, 2):
            s = _textured_settings(host, semantics, max_depth=depth)
            w = _walk(host, dev, osc, s, 0)
            albedo, normal = dev.render_aovs(s, 0)
            _check_walk(w, albedo, normal, "textured, semantics %d, maxDepth %d" % (semantics, depth), s.width)
            ended = w["first_discard"] & ~w["hit"]
            print("maxDepth %d: %d discarded first hits, %d pixels end without a surface" % (depth, w["first_discard"].sum(), ended.sum()))
            assert ended.sum() >= (100 if depth == 1 else 10) and (albedo.reshape(-1, 4)[ended] == 0).all()
            assert (ended == w["first_discard"]).all() if depth == 1 else (ended != w["first_discard"]).any()
    # a BLEND surface is kept by one sample and passed by another
    (d0, b0), (d3, b3) = discards[SAMPLES[0]], discards[SAMPLES[1]]
    assert (b0 & b3 & (d0 != d3)).sum() >= 1


# --------------------------------------------------------------------------------------------------------------------- rule 4
def test_rule_4_temporal_step_reports_the_same_surface(textured, walks):
    host, dev, osc = textured
    for semantics in (PBR, 0):
        s = _textured_settings(host, semantics)
        albedo, normal = dev.render_aovs(s, 0)
        temporal = dev.temporal(s.width, s.height)
        try:
            out = temporal.step(s, np.zeros((s.height, s.width, 3), F), want_aovs=True)
            r0, r1, r2 = temporal.records()
        finally:
            temporal.close()
        assert np.array_equal(out["albedo"], albedo) and np.array_equal(out["normal"], normal), semantics
        hit = albedo[..., 3] > 0.5
        assert np.array_equal(r1[..., 3], normal[..., 3]) and np.array_equal(_encode(r1[..., :3])[hit], normal[..., :3][hit]), semantics
        assert np.array_equal(r2[..., 3].view(np.uint32) != 0xFFFFFFFF, hit) and (r1[~hit] == 0).all() and (r0[~hit] == 0).all(), semantics
        if not semantics:
            continue
        # R0 and R2 name the kept surface: the point lies where the last segment ends, the hit word is that segment's
        _, w, _ = walks(PBR, 0)
        moved = (w["first_discard"] & w["hit"]).reshape(s.height, s.width)
        assert moved.sum() > 50
        unit = w["rays"][:, 3:6].astype(np.float64)
        unit /= np.linalg.norm(unit, axis=1, keepdims=True)
        along = ((r0[..., :3].reshape(-1, 3).astype(np.float64) - w["rays"][:, :3]) * unit).sum(axis=1) / np.linalg.norm(w["rays"][:, 3:6].astype(np.float64), axis=1)
        t = normal[..., 3].reshape(-1).astype(np.float64)
        flat = hit.reshape(-1)
        # (each pass-through starts 1e-4 t off the surface: the sum of the segments is short of the whole by that much)
        assert np.abs(along[flat] - t[flat]).max() < 2e-3 * t[flat].max()
        assert (along[moved.reshape(-1)] > w["first"]["t"][moved.reshape(-1)]).all()
        first_words = dev.temporal(s.width, s.height)
        try:
            first_words.step(_textured_settings(host, 0), np.zeros((s.height, s.width, 3), F))
            plain_r0, _, plain_r2 = first_words.records()
        finally:
            first_words.close()
        same = ~w["first_discard"].reshape(s.height, s.width)
        assert np.array_equal(r2[same].view(np.uint32), plain_r2[same].view(np.uint32)) and np.array_equal(r0[same].view(np.uint32), plain_r0[same].view(np.uint32))
        assert (r2[..., 3].view(np.uint32)[moved] != plain_r2[..., 3].view(np.uint32)[moved]).all()


# --------------------------------------------------------------------------------------------------------------------- invariance
def test_every_node_format_writes_the_same_bits(textured):
    host = textured[0]
    want = {}
    for fname, env, count in T.FORMATS:
        if count:
            continue   # (the counting build is a build of the render kernels; the feature buffers have no counting launch)
        dev = T.upload(host, env)
        try:
            for semantics in (0, PBR | RAY_DIFF):
                s = _textured_settings(host, semantics)
                got = dev.render_aovs(s, 3)
                if semantics not in want:
                    want[semantics] = got
                assert np.array_equal(got[0], want[semantics][0]) and np.array_equal(got[1], want[semantics][1]), (fname, semantics)
        finally:
            dev.close()


def test_a_frame_with_more_pixels_than_the_launch_has_threads(textured):
    """The kernels walk the pixels grid-stride.  The cold launch has 8 blocks of 256 threads per compute unit (csrc/host/hip_backend.cpp
    traceGrid, which ptr_scene_info does not report: the count of compute units is the device's own); the frame is a few rows larger, and
    is compared with ptr_trace_rays and ptr_debug_first_hit_textures where the second lap runs."""
    host, dev, osc = textured
    threads = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    width = 1024
    height = threads // width + 5
    s = _textured_settings(host, PBR, width=width, height=height)
    assert width * height > threads
    albedo, normal = dev.render_aovs(s, 0)
    a, nrm = albedo.reshape(-1, 4), normal.reshape(-1, 4)
    xys = _xys(s, 0)
    rays, _ = pt.debug_camera_rays(s, xys)
    hits = dev.trace_rays(_batch(rays))[0]
    lap = np.arange(threads - 2048, width * height)
    first = dev.first_hit_textures(s, xys[lap])
    settled = ~(first["discard"] > 0)            # a first hit that is kept, or no textured hit at all
    assert np.array_equal(a[lap, 3][settled] > 0.5, hits["t"][lap][settled] >= 0)
    assert np.array_equal(nrm[lap, 3][settled], np.maximum(hits["t"][lap][settled], 0))
    kept = settled & (first["textured"] > 0)
    assert kept.sum() > 500
    assert np.array_equal(a[lap][kept, :3], _clamped(first["base_color"][kept])) and np.array_equal(nrm[lap][kept, :3], _encode(first["normal"][kept]))
    # the first lap: the same pixels' rows of a frame that fits (the camera is the same, the rows are the frame's own)
    everywhere = hits["t"] >= 0
    assert (a[:, 3][everywhere] > 0.5).mean() > 0.95 and not (a[:, 3][~everywhere] > 0.5).any()


def test_without_pbr_the_buffers_are_the_parent_commits():
    """tests/golden/aovs_before_textures.npz: ptr_render_aovs of three scenes as the commit before this rule wrote them (48 x 32, depth 4,
    seed 1337, samples 0 and 3, metalSemantics 0)."""
    golden = np.load(os.path.join(GOLDEN, "aovs_before_textures.npz"))
    for name, assets in (("materials", SCENES), ("cornell_small_mesh", SCENES), ("textured", GOLDEN)):
        host = pt.HostScene.load(os.path.join(GOLDEN, name + ".scene"), assets)
        dev = pt.DeviceScene(host.desc, 0, keepalive=host)
        try:
            s = host.settings_for(width=48, height=32, max_depth=4, seed=1337)
            for sample in SAMPLES:
                albedo, normal = dev.render_aovs(s, sample)
                assert np.array_equal(albedo.view(np.uint32), golden["%s_s%d_albedo" % (name, sample)].view(np.uint32)), (name, sample)
                assert np.array_equal(normal.view(np.uint32), golden["%s_s%d_normal" % (name, sample)].view(np.uint32)), (name, sample)
        finally:
            dev.close()


# --------------------------------------------------------------------------------------------------------------------- what it buys
def test_the_denoiser_is_no_worse_with_the_textured_buffers(textured):
    """The textured fixture at 4 spp under metalSemantics 127, denoised with the buffers of the rule and with those rule 1 alone gives
    (the same settings without PTR_METAL_PBR), against 256 spp of another seed.  The figures are recorded in DESIGN.md section 6a."""
    host, dev, _ = textured
    s = _textured_settings(host, 127)
    image = dev.render_image(s, 4)[0]
    reference = dev.render_image(_textured_settings(host, 127, seed=4242), 256)[0]
    new = dev.render_aovs(s, 0)
    old = dev.render_aovs(_textured_settings(host, 127 & ~PBR), 0)
    rmse = lambda x: float(np.sqrt(np.mean((x.astype(np.float64) - reference.astype(np.float64)) ** 2)))
    with_new, with_old, raw = rmse(pt.denoise(image, *new)), rmse(pt.denoise(image, *old)), rmse(image)
    print("textured 96x72, 4 spp vs 256 spp: RMSE raw %.5f, denoised with rule-1 buffers %.5f, with the textured buffers %.5f" % (raw, with_old, with_new))
    assert with_new <= with_old
