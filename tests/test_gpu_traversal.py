"""The production traversal kernels, ray by ray: k_extend (closest hit) and k_connect (any-hit light connections) against the oracle.

ptr_trace_rays runs the cold one-ray-per-lane loop; every ray of a render goes through the persistent kernels instead (travVote: lane
refill, extra steps without a vote, the HBM spill area past 16 stack levels) with the node format fixed at compile time, by default the
four-wide quantised nodes of travWideStep.  ptr_debug_extend_rays / ptr_debug_connect_rays run those kernels through the render's own
launchers; the tests compare every ray with the oracle, on every node format (the knobs are read at upload, so each scene is uploaded
once per setting), and a failure names the scene, the node format and the first rays that differ.

Thresholds are those of test_ray_queries_match_oracle: hit or miss identical, t identical, the same primitive for 99.9 % of the hits
(the rest are shared-edge ties), u, v within 1e-6 where the mesh triangle agrees and ng identical where the primitive does.  Rays aimed
at vertices and edge midpoints are ties by construction and take no part in the 99.9 %; on a tie (another primitive, or the other half
of a rectangle) t may differ by rounding, at most 1e-5 relative, because the winner of two hits a few ulp apart depends on the order the
walk tests them in.
"""
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as ol
import traversal_ref as tr
import traversal_scenes as ts

pt = ts.pt
pytestmark = pytest.mark.gpu

ORACLE_THREADS = min(16, os.cpu_count() or 1)

# (name, knobs, counting build)
FORMATS = [("default", {}, False), ("PTR_WIDE_NODES=2", {"PTR_WIDE_NODES": "2"}, False), ("PTR_WIDE_NODES=0", {"PTR_WIDE_NODES": "0"}, False),
           ("PTR_QUANTIZED_NODES=0", {"PTR_QUANTIZED_NODES": "0"}, False), ("count=1", {}, True)]


@contextlib.contextmanager
def knobs(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def upload(host, env):
    with knobs(env):
        return pt.DeviceScene(host.desc, 0, keepalive=host)


def oracle(osc, rays, any_hit=False):
    """The oracle's answers, chunks of the batch on ORACLE_THREADS threads (the calls release the GIL)."""
    chunks = np.array_split(rays, max(1, min(ORACLE_THREADS * 4, len(rays) // 512)))
    with ThreadPoolExecutor(ORACLE_THREADS) as ex:
        parts = list(ex.map(lambda c: osc.trace_rays(c, any_hit=any_hit), chunks))
    return np.concatenate(parts) if parts else np.zeros(0, pt.HIT_DTYPE)


def _first(rays, mask, *cols, limit=4):
    idx = np.flatnonzero(mask)[:limit]
    return "; ".join("ray %d %s: %s" % (i, rays[i].tolist(), ", ".join("%s=%r" % (n, c[i]) for n, c in cols)) for i in idx)


def check_extend(where, rays, g, o, ties_only=False, aimed_at_edges=None):
    """k_extend's hits `g` against the oracle's `o` on `rays`; `where` names the scene and node format.  aimed_at_edges: the rays aimed at
    vertices and edge midpoints, ties by construction (they take no part in the 99.9 % of hits on the same primitive)."""
    gh, oh = g["t"] >= 0, o["t"] >= 0
    assert not np.isnan(g["t"]).any(), "%s: k_extend left slots without a hit word: %s" % (
        where, _first(rays, np.isnan(g["t"]), ("word", g["primIndex"])))
    assert np.array_equal(gh, oh), "%s: %d rays hit / miss differently: %s" % (
        where, int((gh != oh).sum()), _first(rays, gh != oh, ("gpu_t", g["t"]), ("oracle_t", o["t"])))
    same = (g["primType"] == o["primType"]) & (g["geomIndex"] == o["geomIndex"]) & (g["primIndex"] == o["primIndex"])
    # a shared-edge tie: another primitive, or another half of the same rectangle (its diagonal; the halves share ng, told apart by u, v)
    du = np.maximum(np.abs(g["u"] - o["u"]), np.abs(g["v"] - o["v"]))
    tie = oh & (~same | ((o["primType"] == 2) & (du > 1e-6)))
    if ties_only:
        tie = np.zeros_like(oh)
    # t bit-identical, except on a shared-edge / shared-vertex tie: there a hit is accepted while T <= |den| * tfar, which lets the later of
    # two triangles whose t differ in the last bits win, so the winner (and its t) depends on the order the walk tests them in
    off = (g["t"] != o["t"]) & ~tie
    assert not off.any(), "%s: %d rays with another t: %s" % (
        where, int(off.sum()), _first(rays, off, ("gpu_t", g["t"]), ("oracle_t", o["t"]), ("gpu_prim", g["primIndex"]), ("oracle_prim", o["primIndex"])))
    rel = np.abs(g["t"] - o["t"]) / np.maximum(np.abs(o["t"]), 1e-30)
    assert (rel[tie] <= 1e-5).all(), "%s: ties further apart than 1e-5: %s" % (where, _first(rays, tie & (rel > 1e-5), ("gpu_t", g["t"]),
                                                                                           ("oracle_t", o["t"])))
    if ties_only or not oh.any():
        return
    general = oh if aimed_at_edges is None else oh & ~aimed_at_edges
    assert same[general].mean() >= 0.999, "%s: %d hits on another primitive: %s" % (
        where, int((~same & general).sum()), _first(rays, ~same & general, ("gpu", g[["primType", "geomIndex", "primIndex"]]),
                                                ("oracle", o[["primType", "geomIndex", "primIndex"]])))
    tri = same & oh & (o["primType"] == 0)
    assert (du[tri] <= 1e-6).all(), "%s: barycentrics differ: %s" % (where, _first(rays, tri & (du > 1e-6), ("du", du)))
    flat = same & oh & ~tie & (o["primType"] != 1)
    assert np.array_equal(g["ng"][flat], o["ng"][flat]), "%s: normals differ: %s" % (
        where, _first(rays, flat & (g["ng"] != o["ng"]).any(axis=1), ("gpu_ng", g["ng"]), ("oracle_ng", o["ng"])))


def run_formats(name, host, rays, o, formats=FORMATS, base_env=None, ties_only=False, want_default=None, aimed_at_edges=None):
    infos = {}
    for fname, env, count in formats:
        dev = upload(host, dict(base_env or {}, **env))
        try:
            g, info = dev.extend_rays(rays, count=count)
        finally:
            dev.close()
        where = "scene %s, node format %s (launched %s)" % (name, fname, pt.DeviceScene.NODE_FORMATS[info["format"]])
        check_extend(where, rays, g, o, ties_only, aimed_at_edges)
        infos[fname] = info
    # the intended instantiation ran
    if "count=1" in infos:
        assert infos["count=1"]["format"] == 3
    if "PTR_QUANTIZED_NODES=0" in infos:
        assert infos["PTR_QUANTIZED_NODES=0"]["format"] == 0
    if "default" in infos:
        if want_default is not None:
            assert infos["default"]["format"] == want_default, (name, infos["default"])
        if infos["default"]["format"] == 2:
            assert infos["PTR_WIDE_NODES=2"]["format"] == 2 and infos["PTR_WIDE_NODES=0"]["format"] == 1, (name, infos)
            assert infos["default"]["wide_depth"] > 0
    return infos


SCENE_IDS = ["A", "B", "C", "D", "D-no-oversize", "E", "G-far", "G-small"]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    cache = {}

    def get(key):
        if key not in cache:
            tmp = tmp_path_factory.mktemp("trav_" + key)
            base = key.split("-")[0]
            host = {"A": ts.scene_a, "B": ts.scene_b, "C": ts.scene_c}.get(base, lambda: None)()
            if base == "D":
                host = ts.scene_d(tmp)
            elif base == "E":
                host = ts.scene_e(tmp)
            elif key == "G-far":
                host = ts.scene_g(tmp, "far")
            elif key == "G-small":
                host = ts.scene_g(tmp, "small")
            cache[key] = (host, tr.Reference(host.desc), ol.OracleScene(host))
        return cache[key]
    return get


def scene_rays(key, host, ref):
    base = key.split("-")[0]
    if base == "E":
        cand, depth = ts.deep_rays(host.desc, ref, 4000, 31)
        rays = np.concatenate([cand[:4000], cand[depth > 16]])
        return rays, depth[depth > 16], np.zeros(len(rays), bool)
    n = {"C": 12000, "D": 6000}.get(base, 8000)
    inside = None
    if len(ref.sph):
        inside = ref.sph[:, :3]
    if base in ("A", "C", "D", "G"):
        # inside the closed blob mesh: the centroid of its vertices
        mesh = ref.tri[ref.src[:, 0] == 0]
        inside = mesh.reshape(-1, 3).mean(axis=0)[None] if inside is None else np.concatenate([inside, mesh.reshape(-1, 3).mean(axis=0)[None]])
    rays, edge = ts.mixed_rays(ref, n, 101, inside, ties=True)
    return rays, None, edge


@pytest.mark.parametrize("key", SCENE_IDS)
def test_extend_matches_oracle_on_every_node_format(scenes, key):
    host, ref, osc = scenes(key)
    rays, depth, edge = scene_rays(key, host, ref)
    o = oracle(osc, rays)
    formats = FORMATS
    base_env = None
    if key == "D-no-oversize":
        # every triangle in the tree and quantised nodes forced: boxes many cells wider than the blob's triangles
        base_env = {"PTR_NO_OVERSIZE": "1", "PTR_QUANTIZED_NODES": "1"}
        formats = [f for f in FORMATS if f[0] != "PTR_QUANTIZED_NODES=0"]
    if key == "C":
        formats = FORMATS + [("PTR_REFILL_BELOW=1", {"PTR_REFILL_BELOW": "1"}, False), ("PTR_REFILL_BELOW=64", {"PTR_REFILL_BELOW": "64"}, False)]
    want = 2 if key.split("-")[0] in ("A", "C", "E", "G") else None
    infos = run_formats(key, host, rays, o, formats, base_env, want_default=want, aimed_at_edges=edge)
    if key == "E":
        # the rays chosen by ptr_debug_walk_stack_depths to hold more than 16 entries went through the spill area and still hit right
        deep = len(depth)
        assert deep > 0 and infos["default"]["stack_limit"] >= int(depth.max()) and infos["default"]["lds_levels"] == 16
        print("scene E: %d of the rays hold more than 16 stack entries, at most %d (stack limit %d)" % (deep, depth.max(),
                                                                                                      infos["default"]["stack_limit"]))


@pytest.mark.parametrize("which", ["triangle", "sphere", "coincident", "flat", "empty"])
def test_extend_on_small_and_degenerate_scenes(tmp_path, which):
    host = ts.scene_f(tmp_path, which)
    osc = ol.OracleScene(host)
    ref = tr.Reference(host.desc)
    rays, edge = ts.mixed_rays(ref, 3000, 202, ref.sph[:, :3] if len(ref.sph) else None, ties=True)
    if which == "flat":
        rays = np.concatenate([rays, ts.grazing_rays(3000, 203)])
        edge = np.concatenate([edge, np.zeros(3000, bool)])
    o = oracle(osc, rays)
    # nine coincident triangles: every hit is a tie, only t and hit or miss are asserted
    run_formats("F-" + which, host, rays, o, ties_only=which == "coincident", aimed_at_edges=edge)
    if which == "empty":
        assert (o["t"] < 0).all()
    else:
        assert (o["t"] >= 0).any()


def test_extend_refills_over_a_large_batch(scenes):
    # 2^21 random rays on the bench scene: the persistent waves refill many times; same t and hit or miss as ptr_trace_rays
    host, ref, _ = scenes("C")
    rays = ts.random_rays(ref, 1 << 21, 303)
    dev = upload(host, {})
    try:
        g, info = dev.extend_rays(rays)
        c, _ = dev.trace_rays(rays)
    finally:
        dev.close()
    assert info["format"] == 2
    check_extend("scene C, 2^21 rays, node format four-wide (against ptr_trace_rays)", rays, g, c, ties_only=True)


CONNECT_FORMATS = [f for f in FORMATS if not f[2]]


@pytest.mark.parametrize("key", ["A", "B", "C", "D", "E"])
def test_connect_matches_oracle_any_hit(scenes, key):
    host, ref, osc = scenes(key)
    rays = scene_rays(key, host, ref)[0][:6000]
    closest = oracle(osc, rays)
    hit = closest["t"] > 0
    rng = np.random.default_rng(404)
    cases = {"tmax=inf": rays}
    r = rays.copy()
    r[:, 7] = np.where(rng.random(len(r)) < 0.5, closest["t"] * rng.uniform(0.2, 1.5, len(r)), rng.uniform(0.01, 2.0, len(r)) *
                       np.abs(r[:, :3]).max()).astype(np.float32)
    r[~np.isfinite(r[:, 7]) | (r[:, 7] <= 2e-4), 7] = 1.0
    cases["random finite tmax"] = r
    r = rays[hit].copy()
    r[:, 7] = closest["t"][hit]                                   # the T <= absDen * tfar boundary
    cases["tmax = closest t"] = r
    r = rays[hit].copy()
    r[:, 7] = np.nextafter(closest["t"][hit], np.float32(0))
    cases["tmax = nextafter(t, 0)"] = r
    expected = {name: oracle(osc, rr, any_hit=True)["t"] >= 0 for name, rr in cases.items()}
    for k, (fname, env, _) in enumerate(CONNECT_FORMATS):
        dev = upload(host, env)
        try:
            for name, rr in cases.items():
                occ, info = dev.connect_rays(rr, records_per_slot=1 + (k + len(name)) % 4)
                where = "scene %s, node format %s (launched %s), %s" % (key, fname, pt.DeviceScene.NODE_FORMATS[info["format"]], name)
                assert np.array_equal(occ, expected[name]), "%s: %d rays occluded differently: %s" % (
                    where, int((occ != expected[name]).sum()), _first(rr, occ != expected[name], ("gpu", occ), ("oracle", expected[name])))
        finally:
            dev.close()
    assert 0.05 < expected["tmax=inf"].mean() < 1.0


LIGHTS = ("camera target=0,2,0 distance=12 yaw=0.3 pitch=0.2 vfov=40\nrenderer maxDepth=4 seed=1337\nbackground solid=0,0,0\n"
          "material type=lambert albedo=0.6,0.6,0.6\nmaterial type=diffuse_light emit=10,10,10\n"
          "rectangle x=-5,5 y=0 z=-5,5 normal=1 material=0\n"
          "sphere center=-1.5,2,0 radius=0.35 material=0\nsphere center=1.4,2.6,0.2 radius=0.45 material=0\n"
          "rectangle x=-0.6,0.4 y=1.8 z=-1,1 normal=1 material=0\n")
LIGHT_LINES = ("rectangle x=-2.5,-0.5 y=4 z=-0.8,0.8 normal=-1 material=1\n", "rectangle x=0.5,2.5 y=4.2 z=-0.6,0.9 normal=-1 material=1\n")


def test_connect_kind3_records_ignore_their_light(tmp_path):
    # a kind-3 record (a specular connection k_shade settled against light i) ignores the two triangles of light i: the same answer as
    # the oracle's any-hit on the scene without that rectangle, for rays aimed at points of light i with tmax = their distance to it
    p = tmp_path / "lights.scene"
    p.write_text(LIGHTS + "".join(LIGHT_LINES))
    host = ts.load(p)
    rng = np.random.default_rng(505)
    n = 4000
    for env in ({}, {"PTR_WIDE_NODES": "0"}, {"PTR_QUANTIZED_NODES": "0"}):
        dev = upload(host, env)
        try:
            assert dev.info()["rect_lights"] == 2
            for i in range(2):
                without = tmp_path / ("without_%d.scene" % i)
                without.write_text(LIGHTS + LIGHT_LINES[1 - i])
                h2 = ts.load(without)
                r = host.desc.rects[2 + i]
                c, eu, ev = (np.array(list(v)[:3], np.float32) for v in (r.corner, r.edgeU, r.edgeV))
                target = c + rng.uniform(0.02, 0.98, (n, 1)).astype(np.float32) * eu + rng.uniform(0.02, 0.98, (n, 1)).astype(np.float32) * ev
                org = np.stack([rng.uniform(-4, 4, n), rng.uniform(0.05, 1.0, n), rng.uniform(-4, 4, n)], axis=1).astype(np.float32)
                dist = np.linalg.norm((target - org).astype(np.float64), axis=1)
                rays = ts.pack(org, ((target - org) / dist[:, None]).astype(np.float32), dist.astype(np.float32))
                want = oracle(ol.OracleScene(h2), rays, any_hit=True)["t"] >= 0
                occ, info = dev.connect_rays(rays, np.full(n, i, np.uint32), records_per_slot=3)
                where = "light scene, knobs %s (launched %s), ignoring light %d" % (env, pt.DeviceScene.NODE_FORMATS[info["format"]], i)
                assert np.array_equal(occ, want), "%s: %d rays differ: %s" % (where, int((occ != want).sum()),
                                                                              _first(rays, occ != want, ("gpu", occ), ("oracle", want)))
                assert 0.05 < want.mean() < 0.95
                # the same rays as kind-0 records stop at light i itself
                occ0, _ = dev.connect_rays(rays, None, records_per_slot=2)
                assert occ0.mean() > want.mean()
        finally:
            dev.close()


def test_probes_reject_rays_the_kernels_cannot_trace(scenes):
    host, ref, _ = scenes("A")
    dev = upload(host, {})
    try:
        rays = ts.random_rays(ref, 16, 606)
        bad = rays.copy()
        bad[3, 3] = 1e-3
        with pytest.raises(pt.PtrError, match="ray 3 has tmin"):
            dev.extend_rays(bad)
        bad = rays.copy()
        bad[5, 7] = 100.0
        with pytest.raises(pt.PtrError, match="ray 5 has tmin"):
            dev.extend_rays(bad)
        with pytest.raises(pt.PtrError, match="ignores light 1 of 1"):
            dev.connect_rays(rays, np.array([0xFFFFFFFF] * 15 + [1], np.uint32))
        with pytest.raises(pt.PtrError, match="records_per_slot"):
            dev.connect_rays(rays, records_per_slot=5)
        e, info = dev.extend_rays(np.zeros((0, 8), np.float32))
        assert e.shape == (0,) and info["format"] == 2 and info["lds_levels"] == 16
    finally:
        dev.close()
