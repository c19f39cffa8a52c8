"""tests/aov_ref.py (rule 1 of the first-hit feature buffers, include/ptr_abi.h ptr_render_aovs) against hand-made pixels, one per branch of
the rule, and its float32 twin against the float64 statement.  Then its material lookup on the oracle's hits of two real scenes, against
the material the oracle's own render loop records at vertex 0 (oracle_path_states).  No GPU."""
import os
from types import SimpleNamespace as NS

import numpy as np

import aov_ref as A
import oracle_lib as ol

pt = ol.pt
GOLDEN = os.path.join(ol.ROOT, "tests", "golden")
SCENES = os.path.join(ol.ROOT, "scenes")


def _material(kind, base):
    return NS(baseColorRoughness=list(base) + [0.5], typeEta=[float(kind), 1.5, 1.5, 0.0])


def _desc(materials):
    return NS(materialCount=len(materials), materials=materials,
              spheres=[NS(materialIndex=[2, 0, 0, 0])], sphereCount=1,
              rects=[NS(materialTwoSided=[1, 0, 0, 0]), NS(materialTwoSided=[7, 1, 0, 0])], rectCount=2,
              meshes=[NS(materialIndex=0), NS(materialIndex=3)], meshCount=2)


MATERIALS = [_material(0, (0.25, 0.5, 0.75)), _material(1, (1.5, -0.25, 0.5)), _material(2, (1.0, 1.0, 1.0)), _material(7, (0.1, 0.2, 0.3))]

# one pixel per branch: (prim type, geom, prim, t, geometric normal, hit shading normal, front face) -> (material, normal before encoding)
S = 1.0 / np.sqrt(2.0)
PIXELS = [
    ("miss", (0, 0, 0, -1.0, (0, 1, 0), (0, 1, 0), 1), None),
    ("mesh, interpolated normal", (0, 0, 5, 2.0, (0, 0, 1), (0, 3, 4), 1), (0, (0, 0.6, 0.8))),
    ("mesh, zero-length normal: the geometric one", (0, 1, 9, 3.0, (0, 1, 0), (0, 0, 0), 1), (3, (0, 1, 0))),
    ("rectangle, material clamped to the table", (2, 0, 1, 4.0, (1, 0, 0), (-1, 0, 0), 0), (3, (-1, 0, 0))),
    ("rectangle, clamped colour", (2, 0, 0, 4.5, (1, 0, 0), (1, 0, 0), 1), (1, (1, 0, 0))),
    ("dielectric sphere, front", (1, 0, 0, 5.0, (S, S, 0), (0, 0, 1), 1), (2, (S, S, 0))),
    ("dielectric sphere, back", (1, 0, 0, 6.0, (S, S, 0), (0, 0, 1), 0), (2, (S, S, 0))),
]


def _rows():
    hits = np.zeros(len(PIXELS), dtype=pt.HIT_DTYPE)
    surf = np.zeros((len(PIXELS), 16), np.float32)
    for i, (_, (kind, geom, prim, t, ng, ns, front), _) in enumerate(PIXELS):
        hits[i]["t"], hits[i]["primType"], hits[i]["geomIndex"], hits[i]["primIndex"] = t, kind, geom, prim
        surf[i, 0], surf[i, 1], surf[i, 5:8], surf[i, 8:11], surf[i, 11] = float(t >= 0), t, ng, ns, front
    return hits, surf


def test_hand_made_pixels_one_per_branch():
    hits, surf = _rows()
    desc = _desc(MATERIALS)
    for semantics in (0, A.FACE_NORMAL):
        for dtype, tol in ((np.float64, 1e-15), (np.float32, 2.0 ** -23)):
            got = A.first_hit_features(desc, hits, surf, semantics, dtype)
            assert got["normal"].dtype == dtype
            for i, (name, _, want) in enumerate(PIXELS):
                if want is None:
                    assert not got["hit"][i] and (got["albedo"][i] == 0).all() and (got["normal"][i] == 0.5).all() and got["distance"][i] == 0, name
                    continue
                material, normal = want
                normal = np.array(normal, np.float64)
                if name == "dielectric sphere, back" and semantics:
                    normal = -normal   # the one pixel PTR_METAL_FACE_NORMAL changes
                base = np.clip(np.array(MATERIALS[material].baseColorRoughness[:3], np.float32), 0, 1)
                assert got["hit"][i] and got["material"][i] == material, name
                assert np.array_equal(got["albedo"][i], base), name
                assert got["distance"][i] == np.float32(hits[i]["t"]), name
                assert np.abs(got["normal"][i] - (normal * 0.5 + 0.5)).max() <= tol, (name, got["normal"][i])
    # the twin sets a tolerance of a few float32 ulps, and the floor holds where the twin happens to be exact
    r64, r32 = (A.first_hit_features(desc, hits, surf, 0, d) for d in (np.float64, np.float32))
    assert A.NORMAL_FLOOR <= A.normal_tolerance(r64, r32) <= 8 * 2.0 ** -23
    assert A.normal_tolerance(r64, r64) == A.NORMAL_FLOOR


def test_a_scene_without_materials_reports_nothing():
    hits, surf = _rows()
    got = A.first_hit_features(_desc([]), hits, surf)
    assert not got["hit"].any() and (got["albedo"] == 0).all() and (got["normal"] == 0.5).all() and (got["distance"] == 0).all()


def test_the_material_lookup_agrees_with_the_oracles_render_loop():
    """hit_materials reads the material of a hit from the scene description; on the materials and textured scenes it names the material
    the oracle's render loop records at vertex 0 (oracle_path_states, tests/path_state_cases.ORACLE_ROW), and the geometric normal of the
    surface record is that vertex's."""
    import path_state_cases as K

    for name, assets in (("materials", SCENES), ("textured", GOLDEN)):
        host = pt.HostScene.load(os.path.join(GOLDEN, name + ".scene"), assets)
        osc = ol.OracleScene(host)
        s = host.settings_for(width=24, height=16, max_depth=2, seed=1337)
        pixels = np.arange(24 * 16, dtype=np.uint32)
        xys = np.stack([pixels % 24, pixels // 24, np.zeros_like(pixels)], axis=1)
        rays, _ = ol.camera_rays(s, xys)
        batch = np.concatenate([rays[:, :3], np.full((len(rays), 1), 1e-4, np.float32), rays[:, 3:], np.full((len(rays), 1), np.inf, np.float32)], axis=1)
        hits = osc.trace_rays(batch, any_hit=False)
        surf = osc.surface_hits(np.concatenate([rays, rays[:, 3:]], axis=1))
        ref = A.first_hit_features(host.desc, hits, surf)
        rows, _ = osc.path_states(s, pixels, 0, 2)
        t = K.oracle_table(rows)
        hit = t["hit"][0] != 0
        assert np.array_equal(hit, ref["hit"]) and hit.sum() > 100, name
        assert np.array_equal(np.minimum(t["material"][0][hit], host.desc.materialCount - 1), ref["material"][hit]), name
        assert np.array_equal(t["normal"][0][hit], surf[hit, 5:8]), name
        assert len(np.unique(ref["material"][hit])) >= 3, name
