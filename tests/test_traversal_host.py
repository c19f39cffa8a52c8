"""Host-side (no GPU) checks behind the traversal tests: the stack depth of the four-wide walk (which rays reach the HBM spill area),
and the oracle the GPU tests compare with, in BVH and brute-force mode, against a float64 brute-force reference (traversal_ref.py).

With test_gpu_traversal.py (GPU == oracle bit for bit) this makes GPU ~= float64.  Thresholds, measured on these scenes and rays:
hit or miss identical except rays within 1e-6 (relative barycentric margin) of a triangle's edge, of a sphere's silhouette, or of tmin;
where both hit and the ray is not grazing (|cos| > 1e-2), |t - t64| <= 1e-5 * max(t64, 1) (measured: at most 3e-6).  The edge margin is
counted in units of what float32 operands resolve (traversal_ref.py) where that is coarser than 1e-6: far or grazing rays.
"""
import numpy as np
import pytest

import oracle_lib as ol
import traversal_ref as tr
import traversal_scenes as ts

pt = ts.pt


def test_hairball_rays_reach_the_spill_area(tmp_path):
    host = ts.scene_e(tmp_path)
    g = pt.debug_scene_geometry(host.desc)
    # the scene keeps its four-wide nodes, and the by-area wide tree fits the stack: 3 x wideDepth + 4 <= kTraversalStackDepth (76), so
    # prepareGeometry's by-level fallback does not run (measured: binary depth 23, wide depth 11)
    assert g["quantized_usable"] == 1 and g["wide_nodes"] > 0 and g["wide_problems"] == 0
    assert 3 * g["wide_depth"] + 4 <= 76, g
    ref = tr.Reference.__new__(tr.Reference)
    ref.tri, ref.sph = np.zeros((0, 3, 3)), np.zeros((0, 4))
    rng = np.random.default_rng(31)
    rays = ts.pack(rng.uniform(-0.2, 1.2, (20000, 3)), ts._unit(rng.normal(size=(20000, 3))))
    depth = pt.walk_stack_depths(host.desc, rays)
    deep = (depth > 16).mean()
    print("scene E: %.1f %% of the rays push more than 16 stack entries, at most %d (wide depth %d)" % (100 * deep, depth.max(), g["wide_depth"]))
    # measured: 32 % of these rays hold more than the 16 LDS levels, at most 26 entries; none past 32
    assert deep >= 0.01
    assert depth.max() <= 3 * g["wide_depth"] + 1
    if depth.max() > 32:
        assert (depth > 32).any()


def test_stack_depth_probe_counts_like_the_device(tmp_path):
    rays = ts.pack(np.random.default_rng(1).uniform(-2, 2, (500, 3)), ts._unit(np.random.default_rng(2).normal(size=(500, 3))))
    # a single triangle: the root reference is a leaf, nothing is pushed; an empty scene walks nothing
    assert (pt.walk_stack_depths(ts.scene_f(tmp_path, "triangle").desc, rays) == 0).all()
    assert (pt.walk_stack_depths(ts.scene_f(tmp_path, "empty").desc, rays) == 0).all()
    # the room keeps its floor out of the tree: the root waits on the stack while the oversize leaf is tested, one entry for every ray
    room = ts.scene_d(tmp_path)
    d = pt.walk_stack_depths(room.desc, ts.pack(np.random.default_rng(3).uniform(-30, 30, (2000, 3)),
                                                ts._unit(np.random.default_rng(4).normal(size=(2000, 3)))))
    assert (d >= 1).all() and d.max() > 1


def _float64_check(name, host, rays):
    ref = tr.Reference(host.desc)
    r64 = ref.trace(rays)
    osc = ol.OracleScene(host)
    for mode in (False, True):
        o = osc.trace_rays(rays, brute_force=mode)
        where = "scene %s, oracle %s" % (name, "brute force" if mode else "BVH")
        clear = (r64["margin"] > 1e-6) & ~r64["near_ends"]
        oh, h64 = o["t"] >= 0, np.isfinite(r64["t"])
        bad = clear & (oh != h64)
        assert not bad.any(), "%s: %d rays hit / miss unlike float64: %s" % (where, int(bad.sum()), [(int(i), rays[i].tolist(), float(o["t"][i]), float(r64["t"][i]))
                                                                                                for i in np.flatnonzero(bad)[:4]])
        # (t of a float32 test is off by about 2^-24 |C| / |cos|: at |cos| 1e-3 that is 6e-5 of t at unit distance, so the t comparison
        # takes the rays with |cos| > 1e-2)
        both = clear & oh & h64 & (r64["cos"] > 1e-2)
        # relative to max(t64, 1), and to what float32 coordinates of that size resolve (scene G far from the origin: 3e4 -> 2e-3)
        scale = np.maximum(np.maximum(r64["t"][both], 1.0), 2.0 ** -24 * np.abs(rays[both, :3]).max(axis=1) / r64["cos"][both] / 1e-5)
        err = np.abs(o["t"][both] - r64["t"][both]) / scale
        assert both.sum() > 0.1 * len(rays) or name.startswith("F-"), (where, both.sum())
        if both.any():
            assert err.max() <= 1e-5, (where, float(err.max()), rays[np.flatnonzero(both)[np.argmax(err)]].tolist())
        print("%s: %d rays, %d left out near a boundary, t relative error at most %.2e" % (where, len(rays), int((~clear).sum()),
                                                                                         float(err.max()) if both.any() else 0.0))


@pytest.mark.parametrize("key", ["A", "B", "D", "F-triangle", "F-sphere", "F-coincident", "F-flat", "F-empty", "G-far", "G-small"])
def test_oracle_matches_float64_reference(tmp_path, key):
    if key == "A":
        host = ts.scene_a()
    elif key == "B":
        host = ts.scene_b()
    elif key == "D":
        host = ts.scene_d(tmp_path)
    elif key.startswith("F-"):
        host = ts.scene_f(tmp_path, key[2:])
    else:
        host = ts.scene_g(tmp_path, key[2:])
    ref = tr.Reference(host.desc)
    n = 300 if key == "D" else 1500
    around = ref
    if key == "D":
        # rays around the blob, not from across the 3000-unit room: a float32 ray from 600 units away cannot place a hit on one of the
        # blob's 0.01-unit triangles to better than about 1e-3 of its size, far outside the 1e-6 margin
        around = tr.Reference.__new__(tr.Reference)
        around.tri, around.sph = ref.tri[ref.src[:, 0] == 0], ref.sph
    rays = ts.mixed_rays(around, n, 11, ref.sph[:, :3] if len(ref.sph) else None)
    if key == "F-flat":
        rays = np.concatenate([rays, ts.grazing_rays(1000, 12)])
    _float64_check(key, host, rays)
