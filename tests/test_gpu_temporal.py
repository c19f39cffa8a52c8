"""Temporal accumulation on the device (include/ptr_temporal.h): k_temporal_accumulate against the numpy restatement
(tests/temporal_ref.py), the records k_surface writes against the rays, the hits and the rows they come from, and whole steps on static
and moving scenes.  Every comparison is exact (array_equal) unless it says otherwise."""
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import deform_scenes as dsc
import temporal_cases as tc
import temporal_ref as ref
import traversal_scenes as ts
from test_gpu_dynamic import compose, matrix_of, rotation
from test_gpu_dynamic_deform import lit_soup_scene
from test_gpu_traversal import knobs

pt = ts.pt
pytestmark = pytest.mark.gpu
F = np.float32
GEOM_MASK = np.uint32((1 << 26) - 1)
SPHERE_BIT = np.uint32(1 << 31)
MISS = np.uint32(0xFFFFFFFF)
FORMATS = [("default", {}), ("PTR_QUANTIZED_NODES=0", {"PTR_QUANTIZED_NODES": "0"})]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def words(a):
    return np.ascontiguousarray(a[..., 3]).view(np.uint32)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    cache = {}

    def get(key):
        if key not in cache:
            tmp = tmp_path_factory.mktemp("temporal_" + key)
            if key == "pair":
                cache[key] = dsc.scene_pair(tmp)
            elif key == "textured":
                cache[key] = pt.HostScene.load(os.path.join(ts.GOLDEN, "textured.scene"), ts.GOLDEN)
            elif key == "lit":
                cache[key] = lit_soup_scene(tmp)
            elif key == "A":
                cache[key] = ts.scene_a()
            elif key == "slide":
                p = tmp / "slide.scene"
                p.write_text("camera target=0,0,0 distance=8 yaw=1.5708 pitch=0 vfov=40\nrenderer maxDepth=3 seed=1337\nbackground solid=0.2,0.2,0.2\n"
                             "material type=lambert albedo=0.7,0.7,0.7\nmaterial type=lambert albedo=0.8,0.3,0.2\n"
                             "material type=diffuse_light emit=6,6,6\n"
                             "rectangle x=-12,12 y=-12,12 z=-2 normal=1 material=0\nrectangle x=-1,1 y=-4,4 z=0 normal=1 material=1\n"
                             "rectangle x=-3,3 y=6 z=2,5 normal=-1 material=2\n")
                cache[key] = ts.load(p, str(tmp))
        return cache[key]
    return get


def settings_of(host, width=48, height=32, seed=1337):
    return host.settings_for(width=width, height=height, max_depth=3, seed=seed)


def upload(host, env=None, dynamic=False):
    with knobs(env or {}):
        return pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=dynamic, deformable=dynamic, primitives=dynamic)


# --------------------------------------------------------------------------------------------------------------------- 1. the kernel alone
def tilted_camera(w, h, origin, yaw):
    """A camera of temporal_cases turned by `yaw` about y and moved to `origin`: not axis-aligned, so no product in the projection is exact."""
    cam = tc.camera(w, h, pixel=1.0 / 48.0)
    c, s = np.cos(yaw), np.sin(yaw)
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    out = np.array([np.zeros(3), r @ cam[1], r @ cam[2], r @ cam[3]])
    out[:2] += np.asarray(origin)
    return out.astype(F)


@pytest.mark.parametrize("size", [(1, 1), (67, 45), (257, 3)], ids=lambda s: "%dx%d" % s)
def test_accumulate_kernel_equals_the_reference(size):
    w, h = size
    cams = (tilted_camera(w, h, (0.1, -0.2, 0.3), 0.05), tilted_camera(w, h, (-0.05, 0.1, 0.2), -0.03))
    behind = tilted_camera(w, h, (0.0, 0.0, -3.0), 0.0)
    cases = [("zero", (0.0, 0.0), cams[0], cams[0], 32), ("integer", (3.0, -2.0), cams[0], cams[0], 32),
             ("integer, maxHistory 1", (3.0, -2.0), cams[0], cams[0], 1), ("fractional", (0.37, 1.62), cams[0], cams[1], 3),
             ("off-image", (w + 5.0, 0.0), cams[0], cams[1], 32), ("two cameras", (-1.25, 0.5), cams[1], cams[0], 32),
             ("behind the camera", (0.0, 0.0), cams[0], cams[0], 32)]
    for k, (name, motion, cam_cur, cam_prev, max_history) in enumerate(cases):
        rgb, cur, prev, history = tc.noisy_case(w, h, 10 * k + w, motion, cam_cur, cam_prev)
        if name == "zero":   # no jitter either: Xprev is X, bit for bit, and the tap is the pixel itself
            cur[2][..., :3] = cur[0][..., :3]
        if name == "behind the camera":   # the points were made in front of cams[0]; the previous camera stands beyond them, looking away
            cam_prev = behind
        for has_history in (True, False):
            p = pt.PtrTemporalParams.defaults(maxHistory=max_history)
            got = pt.debug_temporal_accumulate(rgb, cur, prev, history, cam_cur, cam_prev, p, has_history)
            want = ref.accumulate(rgb, cur, prev, history, cam_cur, cam_prev, max_history=max_history, has_history=has_history)
            for g, x, what in zip(got, want, ("colour", "length", "history")):
                assert g.shape == x.shape and same(g, x), "%s, %s, history %s: %s differs on %d values" % (
                    size, name, has_history, what, int((~((g == x) | (np.isnan(g) & np.isnan(x)))).sum()))
            length = want[1]
            if has_history and w > 1:   # the case is what it says: blends and resets both happen, or only resets where nothing can be found
                hit = (words(cur[2]) != MISS) & np.isfinite(rgb).all(axis=2)
                assert (length[~hit] == 0).all() and (length[hit] >= 1).all()
                if name in ("off-image", "behind the camera"):
                    assert (length[hit] == 1).all(), name
                elif max_history > 1:
                    assert (length[hit] > 1).any() and (length[hit] == 1).any(), name
                else:
                    assert (length[hit] == 1).all() and not same(got[0][hit], rgb[hit]), "maxHistory 1 blends with a = 1: hist + (c - hist)"
                if name == "zero":
                    assert set(np.unique(length[hit])) <= set(range(1, 9)), "one tap of weight 1: integer lengths"
                if name == "fractional":
                    assert (length[hit] == 3).any() and (length <= 3).all()


# --------------------------------------------------------------------------------------------------------------------- 2, 3. the records
def triangle_uv(rows, org, d):
    """traverse.h triangleUv in float32 numpy: rows [n, 3, 4]."""
    v0, e1, e2 = rows[:, 0, :3], rows[:, 1, :3], rows[:, 2, :3]
    ng = ref.cross(e2, e1)
    r = ref.cross(v0 - org, d)
    den = ref.dot(ng, d)
    sgn = np.where(np.signbit(den), F(-1), F(1))
    rcp = F(1) / np.abs(den)
    return (ref.dot(r, e2) * sgn) * rcp, (ref.dot(r, e1) * sgn) * rcp


def expected_records(dev, host, s, now, before):
    """R0, R1.w, R2 as numpy makes them from the camera rays (sample 0), their hits and the downloaded rows `now` / `before`; also the
    rays and the mask of the pixels whose leaf could be named (a rectangle hit on its diagonal fits both halves)."""
    w, h = s.width, s.height
    ys, xs = np.meshgrid(np.arange(h, dtype=np.uint32), np.arange(w, dtype=np.uint32), indexing="ij")
    xys = np.stack([xs.ravel(), ys.ravel(), np.zeros(w * h, np.uint32)], axis=1)
    rays, _ = pt.debug_camera_rays(s, xys)
    org, d = rays[:, :3], rays[:, 3:]
    hits, _ = dev.trace_rays(ts.pack(org, d))
    n = w * h
    tris = now["tris"]
    meta = np.ascontiguousarray(tris[:, 1, 3]).view(np.uint32) if len(tris) else np.zeros(0, np.uint32)
    prim = np.ascontiguousarray(tris[:, 2, 3]).view(np.uint32) if len(tris) else np.zeros(0, np.uint32)
    mesh_leaf = {(int(m & GEOM_MASK), int(p)): i for i, (m, p) in enumerate(zip(meta, prim)) if m >> 30 == 0}
    rect_leaves = {}
    for i, m in enumerate(meta):
        if m >> 30 == 2:
            rect_leaves.setdefault(int(m & GEOM_MASK), []).append(i)
    sphere_leaf = pt.debug_dynamic_tables(host.desc, ["sphereLeaf"])["sphereLeaf"] if host.desc.sphereCount else np.zeros(0, np.uint32)
    word, ident, known = np.full(n, MISS, np.uint32), np.zeros(n, np.uint32), np.ones(n, bool)
    x, x_prev = np.zeros((n, 3), F), np.zeros((n, 3), F)
    t = np.where(hits["t"] >= 0, hits["t"], F(0)).astype(F)
    for i in np.flatnonzero(hits["t"] >= 0):
        kind, geom, index = int(hits["primType"][i]), int(hits["geomIndex"][i]), int(hits["primIndex"][i])
        ident[i] = (kind << 30) | (geom if kind == 0 else index)
        if kind == 1:
            slot = int(sphere_leaf[index])
            word[i] = SPHERE_BIT | np.uint32(slot)
            point = (org[i] + t[i] * d[i])[None]
            x[i] = ref.sphere_point(now["spheres"][slot][None], now["spheres"][slot][None], point)[0]
            x_prev[i] = ref.sphere_point(before["spheres"][slot][None], now["spheres"][slot][None], point)[0]
            continue
        if kind == 0:
            leaf = mesh_leaf[(geom, index)]
        else:
            fits = []   # the half whose barycentrics are the hit's
            for c in rect_leaves[index]:
                cu, cv = triangle_uv(tris[c][None], org[i][None], d[i][None])
                if abs(cu[0] - hits["u"][i]) <= 1e-5 and abs(cv[0] - hits["v"][i]) <= 1e-5:
                    fits.append(c)
            known[i] = len(fits) == 1
            leaf = fits[0] if fits else rect_leaves[index][0]
        word[i] = leaf
        u, v = hits["u"][i:i + 1], hits["v"][i:i + 1]
        x[i] = ref.surface_point(now["tris"][leaf][None], u, v)[0]
        x_prev[i] = ref.surface_point(before["tris"][leaf][None], u, v)[0]
    shape = (h, w)
    return {"word": word.reshape(shape), "id": ident.reshape(shape), "t": t.reshape(shape), "x": x.reshape(h, w, 3), "x_prev": x_prev.reshape(h, w, 3),
            "known": known.reshape(shape), "org": org.reshape(h, w, 3), "dir": d.reshape(h, w, 3)}


def check_records(records, want, what):
    r0, r1, r2 = records
    k = want["known"]
    assert k.mean() > 0.99, what
    hit = want["word"] != MISS
    assert hit.any(), what
    assert np.array_equal(words(r2)[k], want["word"][k]), what
    assert np.array_equal(words(r0), want["id"]) and np.array_equal(r1[..., 3], want["t"]), what
    assert np.array_equal(r0[..., :3][k], want["x"][k]), "%s: X differs on %d pixels" % (what, int((r0[..., :3] != want["x"]).any(axis=2)[k].sum()))
    assert np.array_equal(r2[..., :3][k], want["x_prev"][k]), "%s: Xprev differs on %d pixels" % (what, int((r2[..., :3] != want["x_prev"]).any(axis=2)[k].sum()))
    assert (r0[~hit] == 0).all() and (r1[~hit] == 0).all() and (r2[..., :3][~hit] == 0).all(), what


@pytest.mark.parametrize("fmt", FORMATS, ids=[f[0] for f in FORMATS])
@pytest.mark.parametrize("key", ["pair", "textured", "lit"])
def test_records_of_a_first_step(hosts, key, fmt):
    host = hosts(key)
    dev = upload(host, fmt[1])
    try:
        s = settings_of(host)
        rows = dev.arrays(["tris", "spheres"])
        want = expected_records(dev, host, s, rows, rows)
        temporal = dev.temporal(s.width, s.height)
        rgb = np.random.default_rng(1).random((s.height, s.width, 3)).astype(F)
        out = temporal.step(s, rgb, want_aovs=True)
        assert out["info"]["hadHistory"] == 0 and out["info"]["frameIndex"] == 0 and np.array_equal(out["rgb"], rgb)
        r0, r1, r2 = temporal.records()
        what = "%s, %s" % (key, fmt[0])
        check_records((r0, r1, r2), want, what)
        hit = want["word"] != MISS
        assert np.array_equal(out["length"], hit.astype(F))
        assert np.array_equal(r2[..., :3], r0[..., :3]), "Xprev is X, bit for bit"
        # the AOVs are ptr_render_aovs' own, and the record's normal is the one they encode
        albedo, normal = dev.render_aovs(s, 0)
        assert np.array_equal(out["albedo"], albedo) and np.array_equal(out["normal"], normal), what
        assert np.array_equal((r1[..., :3] * F(0.5) + F(0.5))[hit], normal[..., :3][hit]) and np.array_equal(r1[..., 3], normal[..., 3])
        assert np.array_equal(hit, albedo[..., 3] > 0.5)
        # sanity, not exactness: the interpolated point lies on the ray, to about ten roundings times a conditioning of a hundred
        x, t = r0[..., :3].astype(np.float64), r1[..., 3].astype(np.float64)
        unit = want["dir"] / np.linalg.norm(want["dir"], axis=2, keepdims=True)
        steep = hit & (np.abs(np.sum(unit * r1[..., :3], axis=2)) > np.sin(np.radians(5.0)))
        assert steep.sum() > 0.5 * hit.sum()
        gap = np.linalg.norm(x - (want["org"] + t[..., None] * want["dir"]), axis=2)
        bound = 1e-4 * np.maximum(1.0, np.maximum(np.linalg.norm(x, axis=2), t))
        assert (gap[steep] <= bound[steep]).all(), (what, float((gap / bound)[steep].max()))
        temporal.close()
    finally:
        dev.close()


def updates(host):
    """name -> the update call on a dynamic scene of the `lit` scene"""
    skew = lambda m: (compose((0.3, -0.2, 0.1), rotation((0.3, 1.0, -0.45), 0.4), (1.0, 1.0, 1.0)) @ matrix_of(host, m).astype(np.float64)).astype(F)
    floor = dsc.rect_of(host, 1)
    floor["corner"] = floor["corner"] + np.array([0.4, 0.25, -0.3], F)
    return {"set_mesh_transforms": lambda dev: dev.set_mesh_transforms({0: skew(0), 1: skew(1)}),
            "set_mesh_vertices": lambda dev: dev.set_mesh_vertices({m: dsc.displaced(host, m, 3 + m, collapse=False) for m in range(host.desc.meshCount)}),
            "set_spheres": lambda dev: dev.set_spheres({0: (0.25, 0.3, -0.1, 0.6)}),
            "set_rects": lambda dev: dev.set_rects({1: floor})}


@pytest.mark.parametrize("name", ["set_mesh_transforms", "set_mesh_vertices", "set_spheres", "set_rects"])
def test_records_after_an_update(hosts, name):
    host = hosts("lit")
    dev = upload(host, dynamic=True)
    try:
        s = settings_of(host)
        rgb = np.full((s.height, s.width, 3), 0.5, F)
        temporal = dev.temporal(s.width, s.height)
        temporal.step(s, rgb)
        before = dev.arrays(["tris", "spheres"])
        updates(host)[name](dev)
        after = dev.arrays(["tris", "spheres"])
        assert not (np.array_equal(before["tris"], after["tris"]) and np.array_equal(before["spheres"], after["spheres"]))
        info = temporal.step(s, rgb)["info"]
        assert info["hadHistory"] == 1 and info["frameIndex"] == 1 and info["snapshotMs"] > 0
        records = temporal.records()
        want = expected_records(dev, host, s, after, before)
        check_records(records, want, name)
        moved = (records[0][..., :3] != records[2][..., :3]).any(axis=2)
        assert moved.any() and not moved.all(), "something moved, something stayed"
        # no update between two steps: the snapshot holds the rows the rays meet
        temporal.step(s, rgb)
        r0, _, r2 = temporal.records()
        assert np.array_equal(r0[..., :3], r2[..., :3]) and np.array_equal(r0, records[0])
        temporal.close()
    finally:
        dev.close()


def test_a_static_scene_never_moves(hosts):
    host = hosts("lit")
    dev = upload(host)
    try:
        assert not dev.is_dynamic
        s = settings_of(host)
        temporal = dev.temporal(s.width, s.height)
        for k in range(3):
            s.seed = 100 + k
            info = temporal.step(s, np.full((s.height, s.width, 3), 0.5, F))["info"]
            r0, _, r2 = temporal.records()
            assert np.array_equal(r0[..., :3], r2[..., :3]) and info["snapshotMs"] == 0 and info["frameIndex"] == k
        temporal.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 4. a static sequence
def test_static_sequence_is_the_running_mean(hosts):
    """Static scene, fixed camera, six frames of 2 spp with different seeds.  The seed moves the ray of sample 0 inside its pixel, so at a
    silhouette a pixel can show another surface (or none) than in the frame before, and the filter resets it, as it must.  The running
    mean is therefore held on the pixels whose own tap counts in every frame by the header's step 5 (same id, cosine, plane distance -
    three lines of numpy on the downloaded records), which must be at least 80 % of the image; and every pixel of every frame, the reset
    ones included, is held to the reference fed the downloaded records, in test 5's way."""
    host = hosts("A")
    dev = upload(host)
    try:
        w, h = 67, 45
        temporal = dev.temporal(w, h)
        p = pt.PtrTemporalParams.defaults()
        frames, lengths, outs, recs = [], [], [], []
        for k in range(6):
            s = settings_of(host, w, h, seed=500 + k)
            frames.append(dev.render_image(s, 2)[0])
            out = temporal.step(s, frames[-1])
            outs.append(out["rgb"])
            lengths.append(out["length"])
            recs.append(temporal.records())
            assert np.array_equal(recs[-1][0][..., :3], recs[-1][2][..., :3])
        cam = pt.debug_temporal_camera(settings_of(host, w, h))
        steady = (words(recs[0][2]) != MISS) & np.isfinite(frames[0]).all(axis=2)
        never = ~steady
        mean = frames[0].copy()
        assert np.array_equal(outs[0], frames[0])
        want = ref.accumulate(frames[0], recs[0], recs[0][:2], np.zeros((h, w, 4), F), cam, cam, has_history=False)
        assert same(outs[0], want[0]) and np.array_equal(lengths[0], want[1])
        for k in range(1, 6):
            (r0, r1, r2), (q0, q1, _) = recs[k], recs[k - 1]
            want = ref.accumulate(frames[k], recs[k], recs[k - 1][:2], want[2], cam, cam)
            assert same(outs[k], want[0]) and np.array_equal(lengths[k], want[1]), "frame %d against the reference, every pixel" % k
            hit = (words(r2) != MISS) & np.isfinite(frames[k]).all(axis=2)
            to_camera = r2[..., :3] - cam[0]
            counts = hit & (words(q0) == words(r0)) & (ref.dot(q1[..., :3], r1[..., :3]) >= F(p.normalCos)) & \
                (np.abs(ref.dot(r2[..., :3] - q0[..., :3], q1[..., :3])) <= F(p.planeTolerance) * np.sqrt(ref.dot(to_camera, to_camera)))
            steady &= counts
            never &= ~hit
            mean = mean + (frames[k] - mean) * (F(1) / F(k + 1))
            assert np.array_equal(outs[k][steady], mean[steady]) and (lengths[k][steady] == k + 1).all(), k
            assert np.array_equal(outs[k][never], frames[k][never]) and (lengths[k][never] == 0).all(), k
        # How much of the image that must be: only a pixel that an id boundary or the silhouette crosses can change surface when the ray
        # moves inside it, and scene A at 67 x 45 shows the box's opening, its inner edges, the light and the mesh's outline - some nine
        # lines of at most the image's width, 600 of its 3,015 pixels: a fifth of the image at most.
        settled = float((steady | never).mean())
        print("settled pixels: %.3f (hit in every frame %.3f, miss in every frame %.3f)" % (settled, steady.mean(), never.mean()))
        assert settled >= 0.8
        assert np.allclose(outs[5][steady], np.mean(frames, axis=0)[steady], atol=1e-5)
        temporal.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 5. whole steps with motion
@pytest.mark.parametrize("motion", ["mesh", "yaw", "dolly"])
def test_steps_equal_the_reference_fed_the_records(hosts, motion):
    host = hosts("lit")
    dev = upload(host, dynamic=True)
    try:
        temporal = dev.temporal(48, 32, pt.PtrTemporalParams.defaults(maxHistory=2))
        history, prev, cam_prev = np.zeros((32, 48, 4), F), None, None
        blended = 0
        for k in range(3):
            s = settings_of(host, seed=40 + k)
            if motion == "mesh" and k:
                turn = rotation((0.0, 1.0, 0.0), np.radians(8.0 * k))
                dev.set_mesh_transforms({0: (matrix_of(host, 0).astype(np.float64) @ turn).astype(F)})
            elif motion == "yaw":
                s.cameraYaw += float(np.radians(1.0) * k)
            elif motion == "dolly":
                s.cameraDistance *= float(1.0 - 0.03 * k)
            rgb = dev.render_image(s, 1)[0]
            out = temporal.step(s, rgb)
            records = temporal.records()
            cam = pt.debug_temporal_camera(s)
            want = ref.accumulate(rgb, records, prev if k else records[:2], history, cam, cam_prev if k else cam, max_history=2, has_history=k > 0)
            assert same(out["rgb"], want[0]) and np.array_equal(out["length"], want[1]), (motion, k)
            blended += int((want[1] == 2).sum()) if k else 0
            if k:
                hit = want[1] > 0
                shift = np.abs(ref.project(cam_prev, records[2][..., :3], 48, 32)[0] - ref.project(cam, records[0][..., :3], 48, 32)[0])
                assert shift[hit].max() > 0.1, "the image moved"
            history, prev, cam_prev = want[2], records[:2], cam
        assert blended > 48 * 32 // 4, "and most of it found its history"
        temporal.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 6. disocclusion
def test_disocclusion_resets_what_the_rectangle_uncovered(hosts):
    host = hosts("slide")
    dev = upload(host, dynamic=True)
    try:
        w, h = 96, 64
        s = settings_of(host, w, h)
        cam = pt.debug_temporal_camera(s).astype(np.float64)
        pixel_width = np.linalg.norm(cam[2]) / w   # of the plane z = 0, which is where the camera's focus plane lies (distance 8)
        assert abs(np.linalg.norm(cam[0]) - 8.0) < 1e-5
        temporal = dev.temporal(w, h)
        first, second = dev.render_image(s, 1)[0], None
        temporal.step(s, first)
        before = words(temporal.records()[0])
        slider = dsc.rect_of(host, 1)
        slider["corner"] = slider["corner"] + np.array([8.0 * pixel_width, 0.0, 0.0], F)
        dev.set_rects({1: slider})
        second = dev.render_image(s, 1)[0]
        out = temporal.step(s, second)
        after = words(temporal.records()[0])
        wall, rect = np.uint32(2 << 30), np.uint32(2 << 30 | 1)
        assert set(np.unique(before)) == set(np.unique(after)) == {wall, rect}
        # the band: within 2 px of a vertical edge of the rectangle in either frame
        band = np.zeros(w, bool)
        for mask in (before == rect, after == rect):
            cols = np.flatnonzero(mask.any(axis=0))
            assert len(cols) == cols[-1] - cols[0] + 1 and 20 <= len(cols) <= 24
            for edge in (cols[0] - 0.5, cols[-1] + 0.5):   # between the last column outside and the first inside
                band |= np.abs(np.arange(w) + 0.5 - (edge + 0.5)) <= 2.0
        assert abs(abs(int(np.flatnonzero((after == rect).any(axis=0))[0]) - int(np.flatnonzero((before == rect).any(axis=0))[0])) - 8) <= 1
        assert band.mean() <= 0.25
        keep = np.broadcast_to(~band, (h, w))
        uncovered = keep & (before == rect) & (after == wall)
        both = keep & (before == wall) & (after == wall)
        inside = keep & (after == rect)
        assert uncovered.sum() >= 3 * h and both.sum() > 0.4 * w * h and inside.sum() >= 12 * h   # 22 columns less its own two edges' and the old right edge's bands
        assert (out["length"][uncovered] == 1).all() and np.array_equal(out["rgb"][uncovered], second[uncovered])
        assert (out["length"][both] == 2).all() and (out["length"][inside] == 2).all()
        assert np.array_equal(out["rgb"][both], first[both] + (second[both] - first[both]) * F(0.5))
        temporal.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 7. reset and refusals
def test_reset_and_refusals_leave_the_history_alone(hosts):
    host = hosts("pair")
    dev = upload(host)
    try:
        s = settings_of(host)
        rng = np.random.default_rng(3)
        frames = rng.random((3, s.height, s.width, 3)).astype(F)
        plain, refused = dev.temporal(s.width, s.height), dev.temporal(s.width, s.height)
        want = [plain.step(s, f) for f in frames[:2]]
        assert want[1]["info"]["hadHistory"] == 1 and (want[1]["length"] == 2).any()
        lib = pt.load_library()
        err = C.create_string_buffer(256)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        out = np.zeros_like(frames[0])
        assert same(refused.step(s, frames[0])["rgb"], want[0]["rgb"])
        other = settings_of(host, s.width + 1, s.height)
        assert lib.ptr_temporal_step(refused._h, C.byref(other), fp(frames[1]), fp(out), None, None, None, None, err, len(err)) == 1
        assert err.value.startswith(b"ptr_temporal_step: the settings are 49x32")
        assert lib.ptr_temporal_step(refused._h, C.byref(s), None, fp(out), None, None, None, None, err, len(err)) == 1 and b"null argument" in err.value
        assert lib.ptr_temporal_step_device(refused._h, C.byref(s), None, C.c_void_p(out.ctypes.data), None, None, None, None, None, err, len(err)) == 1
        assert err.value == b"ptr_temporal_step_device: null argument"
        host_pointer = C.c_void_p(frames[1].ctypes.data)
        assert lib.ptr_temporal_step_device(refused._h, C.byref(s), host_pointer, host_pointer, None, None, None, None, None, err, len(err)) == 1
        assert err.value.startswith(b"ptr_temporal_step_device: d_rgb is") and b"not" in err.value
        with pytest.raises(pt.PtrError, match="maxHistory"):
            dev.temporal(s.width, s.height, pt.PtrTemporalParams.defaults(maxHistory=0))
        with pytest.raises(pt.PtrError, match="non-zero"):
            dev.temporal(0, s.height)
        got = refused.step(s, frames[1])
        assert got["info"]["frameIndex"] == 1 and same(got["rgb"], want[1]["rgb"]) and np.array_equal(got["length"], want[1]["length"])
        # reset: the next step is a first step
        refused.reset()
        with pytest.raises(pt.PtrError, match="no step"):
            refused.records()
        again = refused.step(s, frames[2])
        assert again["info"]["hadHistory"] == 0 and again["info"]["frameIndex"] == 0 and np.array_equal(again["rgb"], frames[2])
        assert np.array_equal(again["length"], want[0]["length"])
        plain.close()
        refused.close()
        with pytest.raises(pt.PtrError, match="closed"):
            refused.step(s, frames[0])
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 8. host and device entry points
def test_host_and_device_steps_agree(hosts):
    host = hosts("lit")
    dev = upload(host)
    try:
        s = settings_of(host)
        h, w = s.height, s.width
        frames = np.random.default_rng(5).random((3, h, w, 3)).astype(F)
        on_host, on_device, on_stream = (dev.temporal(w, h) for _ in range(3))
        side = torch.cuda.Stream(device=0)
        for k, frame in enumerate(frames):
            s.seed = 70 + k
            want = on_host.step(s, frame, want_aovs=True)
            rgb = torch.from_numpy(frame).cuda()
            outs = {name: torch.zeros((h, w, c), dtype=torch.float32, device="cuda:0") for name, c in (("rgb", 3), ("length", 1), ("albedo", 4), ("normal", 4))}
            info = on_device.step_device(s, rgb, outs["rgb"], outs["length"], outs["albedo"], outs["normal"], want_info=True)
            assert info["frameIndex"] == k and info["surfaceMs"] > 0 and info["accumulateMs"] > 0
            torch.cuda.synchronize()
            for name in outs:
                assert same(outs[name].cpu().numpy().reshape(want[name].shape), want[name]), (k, name)
            # on a side stream, behind the kernels that produce rgb there, and in place
            with torch.cuda.stream(side):
                half = torch.from_numpy(frame * F(0.5)).cuda(non_blocking=False)
                produced = half + half   # exact: the frame again, made on `side`
                length = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
                assert on_stream.step_device(s, produced, out_length=length) is None
            side.synchronize()
            assert same(produced.cpu().numpy(), want["rgb"]) and np.array_equal(length.cpu().numpy(), want["length"]), k
        with pytest.raises(pt.PtrError, match="not a torch tensor"):
            on_device.step_device(s, frames[0])
        # the same buffer in and out is allowed (above); one that overlaps it at an offset is refused, with the history as it was
        big = torch.zeros(h * w * 3 + 3, dtype=torch.float32, device="cuda:0")
        with pytest.raises(pt.PtrError, match="overlap"):
            on_device.step_device(s, big[:h * w * 3], big[3:])
        s.seed = 99
        frame = torch.from_numpy(frames[0]).cuda()
        on_device.step_device(s, frame)
        torch.cuda.synchronize()
        assert same(frame.cpu().numpy(), on_host.step(s, frames[0])["rgb"])
        with pytest.raises(pt.PtrError, match="contiguous float32"):
            on_device.step_device(s, torch.zeros((h, w, 4), device="cuda:0"))
        for t in (on_host, on_device, on_stream):
            t.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 9. the scene is untouched
@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_the_scene_is_untouched(hosts, dynamic):
    host = hosts("lit")
    dev = upload(host, dynamic=dynamic)
    try:
        s = settings_of(host)
        digest = lambda: {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in dev.arrays().items()}
        before, image = digest(), dev.render_image(s, 2)[0]
        temporal = dev.temporal(s.width, s.height)
        for k in range(3):
            temporal.step(s, image, want_aovs=True)
        assert digest() == before
        assert np.array_equal(dev.render_image(s, 2)[0], image)
        temporal.close()
        assert digest() == before
    finally:
        dev.close()
