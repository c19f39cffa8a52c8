"""include/ptr_deform.h on the device: ptr_scene_set_mesh_vertices, ptr_scene_set_spheres and ptr_scene_set_rects against what a fresh
upload of the changed description produces.  Every comparison of arrays and images is exact (bit patterns); the ray-by-ray comparisons
with the oracle use check_extend of test_gpu_traversal.py with that file's own thresholds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deform_scenes as dsc
import dynamic_ref as dr
import oracle_lib as ol
import traversal_ref as tr
import traversal_scenes as ts
from test_gpu_dynamic import FORMATS, FORMAT_IDS, by_meta, matrix_of, same_arrays, small_settings, soup_scene, t1_t2
from test_gpu_traversal import check_extend, knobs, oracle

pt = ts.pt
pytestmark = pytest.mark.gpu

GOLDEN = ts.GOLDEN
MESH_SCENES = ["F-triangle", "pair", "strip", "F-coincident", "textured", "A", "soup"]
LIGHT, WALL = 5, 1   # rectangles of scene A: the light in the ceiling, the red wall


def upload(holder, env=None, dynamic=True, deformable=True, primitives=True):
    with knobs(env or {}):
        return pt.DeviceScene(holder.desc, 0, keepalive=holder, dynamic=dynamic, deformable=dynamic and deformable, primitives=dynamic and primitives)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    cache = {}

    def get(key):
        if key not in cache:
            tmp = tmp_path_factory.mktemp("deform_" + key.replace("-", "_"))
            if key == "textured":
                cache[key] = pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN)
            elif key == "A":
                cache[key] = ts.scene_a()
            elif key == "D":
                cache[key] = ts.scene_d(tmp)
            elif key == "soup":
                cache[key] = soup_scene(tmp)
            elif key == "lit":
                cache[key] = lit_soup_scene(tmp)
            elif key == "pair":
                cache[key] = dsc.scene_pair(tmp)
            elif key == "strip":
                cache[key] = dsc.scene_strip(tmp)
            else:
                cache[key] = ts.scene_f(tmp, key[2:])
        return cache[key]
    return get


def lit_soup_scene(tmp):
    """The tie-free soup of test_gpu_dynamic.py under a rectangle light, over a floor rectangle and beside a sphere: no two primitives
    share an edge or touch, so a refitted tree and a fresh one find the same hits."""
    soup_scene(tmp)
    p = tmp / "lit.scene"
    p.write_text("camera target=0,0,0 distance=8 yaw=1.5708 pitch=0.25 vfov=40\nrenderer maxDepth=4 seed=1337\nbackground\n"
                 "material type=lambert albedo=0.7,0.5,0.3\nmaterial type=metal albedo=0.8,0.8,0.9 fuzz=0.1\n"
                 "material type=diffuse_light emit=12,11,10\n"
                 "rectangle x=-1,1 y=2.5 z=-0.8,0.8 normal=-1 material=2\nrectangle x=-4,4 y=-1.2 z=-3,3 normal=1 material=0\n"
                 "sphere center=0,0.1,0.1 radius=0.45 material=1\n"
                 "mesh path=soup_a.obj translate=-2,0,0 material=0\nmesh path=soup_b.obj translate=2,0,0 material=1\n")
    return ts.load(p, str(tmp))


def deformations(host, seed=3, collapse=True):
    return {m: dsc.displaced(host, m, seed + m, collapse) for m in range(host.desc.meshCount)}


def originals(host):
    return {m: dsc.original(host, m) for m in range(host.desc.meshCount)}


def tree_follows_the_bounds(host, got, info, what):
    """boxes, grid, qnodes and wnodes equal dynamic_ref's refit of the downloaded bounds on the upload's topology."""
    t = pt.debug_dynamic_tables(host.desc, ["schedule", "levelOffsets", "wideSource"])
    boxes = dr.refit(got["boxes"], t["schedule"], t["levelOffsets"], got["triBounds"], got["sphereBounds"])
    same_arrays({"boxes": got["boxes"]}, {"boxes": boxes}, what + " (refit reference)")
    if not len(got["boxes"]):
        return
    lo, hi = dr.root_box(got["boxes"])
    grid = dr.grid_of(lo, hi)
    same_arrays({"grid": got["grid"]}, {"grid": grid}, what)
    assert np.array_equal(np.array(info["sceneLo"], np.float32), lo) and np.array_equal(np.array(info["sceneHi"], np.float32), hi)
    if len(got["qnodes"]):
        q = dr.quantise(got["boxes"], grid)
        assert np.array_equal(got["qnodes"], q), what
        if len(got["wnodes"]):
            assert np.array_equal(got["wnodes"], dr.wide_copy(got["wnodes"], q, t["wideSource"])), what


def same_by_meta(got, want, what, names=("tris", "triNormals", "triUv", "triTangent", "triBounds")):
    go, wo = by_meta(got), by_meta(want)
    for name in names:
        assert len(got[name]) == len(want[name]), (what, name)
        if len(got[name]):
            a, b = got[name][go].view(np.uint32), want[name][wo].view(np.uint32)
            assert np.array_equal(a, b), "%s: %s differs on %d triangles, first %s" % (
                what, name, int((a != b).any(axis=(1, 2)).sum()), np.flatnonzero((a != b).any(axis=(1, 2)))[:4])


# --------------------------------------------------------------------------------------------------------------------- 1. deform and restore
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("key", MESH_SCENES)
def test_deform_and_restore(hosts, key, fmt):
    host = hosts(key)
    dev = upload(host, fmt[1])
    try:
        assert dev.is_dynamic and dev.dynamic_flags == 3
        first = dev.arrays()
        s = small_settings(host)
        before = dev.render_image(s, 4)[0]
        info = dev.set_mesh_vertices(deformations(host))
        assert info["trianglesMoved"] == sum(host.desc.meshes[m].indexCount // 3 for m in range(host.desc.meshCount))
        moved = dev.arrays()
        for name in ("tris", "triNormals", "triBounds", "objPos", "objNrm"):
            assert not np.array_equal(moved[name], first[name]), name
        assert np.array_equal(moved["objPos"][..., 3].view(np.uint32), first["objPos"][..., 3].view(np.uint32)), "the w words of objPos stay"
        assert np.isfinite(dev.render_image(s, 1)[0]).all()
        dev.set_mesh_vertices(originals(host))
        same_arrays(dev.arrays(), first, "scene %s, %s, after the restore" % (key, fmt[0]))
        assert np.array_equal(dev.render_image(s, 4)[0], before)
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 2. fresh upload
@pytest.mark.parametrize("key", MESH_SCENES)
def test_deformed_arrays_equal_a_fresh_uploads(hosts, key):
    host = hosts(key)
    new = deformations(host, seed=9)
    dev, fresh = upload(host), upload(dsc.Changed(host, vertices=new))
    try:
        info = dev.set_mesh_vertices(new)
        got, want = dev.arrays(), fresh.arrays()
        what = "scene %s deformed" % key
        same_by_meta(got, want, what)
        if key == "textured":
            assert len(got["triUv"]) and len(got["triTangent"]) and len(got["objTan"])
        tree_follows_the_bounds(host, got, info, what)
        # a rigid move on top: the bake reads the gathered corners, not the upload's
        last = host.desc.meshCount - 1
        m = t1_t2(host, last)[1]
        moved = upload(dsc.Changed(host, vertices=new, matrices={last: m}))
        try:
            info = dev.set_mesh_transforms({last: m})
            got = dev.arrays()
            same_by_meta(got, moved.arrays(), what + " and moved")
            tree_follows_the_bounds(host, got, info, what + " and moved")
            # and a deformation after the move bakes under the matrix the mesh has now
            newer = deformations(host, seed=21)
            dev.set_mesh_vertices({last: newer[last]})
            again = upload(dsc.Changed(host, vertices={**new, last: newer[last]}, matrices={last: m}))
            try:
                same_by_meta(dev.arrays(), again.arrays(), what + ", moved and deformed again")
            finally:
                again.close()
        finally:
            moved.close()
    finally:
        dev.close()
        fresh.close()


# --------------------------------------------------------------------------------------------------------------------- 3. spheres and rectangles
SPHERE_TO = (150.0, 300.0, 420.0, 55.0)
LIGHT_TO = dict(corner=(120.0, 554.0, 150.0), edgeU=(0.0, 0.0, 105.0), edgeV=(130.0, 0.0, 0.0), normal=(0.0, -1.0, 0.0))   # edgeU x edgeV = +y: flipped
WALL_TO = dict(corner=(-20.0, -10.0, 0.0), edgeU=(0.0, 565.0, 0.0), edgeV=(10.0, 0.0, 555.0), normal=(1.0, 0.0, 0.0))


def primitive_rows(arrays, rect=None, sphere=None):
    """The rows of one rectangle / one sphere in downloaded arrays, found by index and by meta word."""
    out = {}
    if rect is not None:
        out["rects"] = arrays["rects"][rect]
        lights = arrays["rectLights"].view(np.uint32)
        for li in np.flatnonzero(lights[:, 2, 3] == rect):
            out["rectLights"] = arrays["rectLights"][li]
        w = arrays["tris"].view(np.uint32)
        for half in range(2):
            k = np.flatnonzero((w[:, 1, 3] >> 30 == 2) & (w[:, 1, 3] & 0x3FFFFFF == rect) & (w[:, 2, 3] == 2 * rect + half))
            assert len(k) == 1
            for name in ("tris", "triNormals", "triBounds"):
                out[(name, half)] = arrays[name][k[0]]
    if sphere is not None:
        return out, sphere
    return out, None


def test_moved_spheres_and_rectangles_equal_a_fresh_uploads(hosts):
    host = hosts("A")
    dev = upload(host)
    try:
        first = dev.arrays()
        state = {"spheres": {}, "rects": {}}
        light, wall = pt.rect_update(LIGHT, **LIGHT_TO), pt.rect_update(WALL, **WALL_TO)
        assert np.dot(np.cross(LIGHT_TO["edgeU"], LIGHT_TO["edgeV"]), LIGHT_TO["normal"]) < 0, "the light's winding flips"
        steps = [("sphere", lambda: dev.set_spheres({0: SPHERE_TO}), lambda: state["spheres"].update({0: SPHERE_TO}), None),
                 ("light", lambda: dev.set_rects({LIGHT: LIGHT_TO}), lambda: state["rects"].update({LIGHT: light}), LIGHT),
                 ("wall", lambda: dev.set_rects({WALL: WALL_TO}), lambda: state["rects"].update({WALL: wall}), WALL)]
        for name, call, note, rect in steps:
            info = call()
            note()
            assert info["trianglesMoved"] == (2 if rect is not None else 0)
            fresh = upload(dsc.Changed(host, spheres=state["spheres"], rects=state["rects"]))
            try:
                got, want = dev.arrays(), fresh.arrays()
                what = "scene A after moving the " + name
                if rect is None:
                    # spheres by original index: through the leaf slots of either scene
                    slot_got = pt.debug_dynamic_tables(host.desc, ["sphereLeaf"])["sphereLeaf"][0]
                    slot_want = pt.debug_dynamic_tables(fresh._keepalive.desc, ["sphereLeaf"])["sphereLeaf"][0]
                    for arr in ("spheres", "sphereBounds"):
                        assert np.array_equal(got[arr][slot_got].view(np.uint32), want[arr][slot_want].view(np.uint32)), (what, arr)
                    assert np.array_equal(got["spheres"][slot_got], np.array(SPHERE_TO, np.float32))
                else:
                    a, b = primitive_rows(got, rect)[0], primitive_rows(want, rect)[0]
                    assert set(a) == set(b) and (("rectLights" in a) == (rect == LIGHT))
                    for k in b:
                        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)
                # everything else, too: every triangle and every rects / rectLights row
                same_by_meta(got, want, what, names=("tris", "triNormals", "triBounds"))
                same_arrays(got, want, what, names=("rects", "rectLights"))
                tree_follows_the_bounds(host, got, info, what)
            finally:
                fresh.close()
        r0, r1 = dsc.rect_of(host, LIGHT), dsc.rect_of(host, WALL)
        dev.set_rects({LIGHT: r0, WALL: r1})
        dev.set_spheres({0: list(host.desc.spheres[0].centerRadius)})
        same_arrays(dev.arrays(), first, "scene A after moving everything back")
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 4. hits
def waved(host, mesh=0, phase=0.0):
    """A sinusoidal displacement along the normals, a tenth of the mesh's box high."""
    pos, nrm, tan, _ = dsc.mesh_data(host, mesh)
    box = float(np.max(pos.max(axis=0) - pos.min(axis=0)))
    k = 9.0 / box
    h = (0.1 * box * np.sin(k * pos[:, 0] + phase) * np.cos(k * pos[:, 2] - 0.5 * phase)).astype(np.float32)
    out = ((pos + nrm * h[:, None]).astype(np.float32), nrm)
    return out if tan is None else out + (tan,)


@pytest.mark.parametrize("key", ["A", "D"])
def test_hits_after_the_updates_equal_the_oracles(hosts, key):
    host = hosts(key)
    new = {0: waved(host)}
    if key == "A":
        spheres, rects = {0: SPHERE_TO}, {LIGHT: LIGHT_TO, WALL: WALL_TO}
    else:   # the room: its light, lowered and turned over a corner
        spheres, rects = {}, {1: dict(corner=(-30.0, 60.0, -20.0), edgeU=(70.0, 10.0, 0.0), edgeV=(0.0, 5.0, 60.0), normal=(0.1, -1.0, 0.0))}
    changed = dsc.Changed(host, vertices=new, spheres=spheres, rects={i: pt.rect_update(i, **r) for i, r in rects.items()})
    ref, osc = tr.Reference(changed.desc), ol.OracleScene(changed)
    rays, edge = ts.mixed_rays(ref, 20000, 707, ties=True)
    o = oracle(osc, rays)
    assert (o["t"] >= 0).any()
    for fname, env in FORMATS:
        dev = upload(host, env)
        try:
            dev.set_mesh_vertices(new)
            if spheres:
                dev.set_spheres(spheres)
            dev.set_rects(rects)
            c, _ = dev.trace_rays(rays)
            check_extend("scene %s deformed and moved, %s, ptr_trace_rays" % (key, fname), rays, c, o, aimed_at_edges=edge)
        finally:
            dev.close()


# --------------------------------------------------------------------------------------------------------------------- 5. renders
def assert_same_image(got, want, what):
    assert want.max() > 0 and np.isfinite(want).all()
    diff = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not diff.any(), "%s: %d pixels differ, first %s" % (what, int(diff.sum()), [
        (int(x), int(y), got[y, x].tolist(), want[y, x].tolist()) for y, x in list(zip(*np.nonzero(diff)))[:4]])


@pytest.mark.parametrize("metal", [0, pt.PTR_METAL_FACE_NORMAL | pt.PTR_METAL_SPECULAR | pt.PTR_METAL_CLAMPS], ids=["default", "metal"])
def test_render_of_a_deformed_scene_equals_a_fresh_uploads(hosts, metal):
    host = hosts("soup")
    states = [{m: waved(host, m, phase) for m in range(2)} for phase in (0.4, 1.7, 2.9)]
    s = small_settings(host, 64, 48, 4, metal)
    dev, fresh = upload(host), upload(dsc.Changed(host, vertices=states[2]), dynamic=False)
    try:
        for state in states:
            dev.set_mesh_vertices(state)
        assert_same_image(dev.render_image(s, 4)[0], fresh.render_image(s, 4)[0], "the soup deformed three times")
    finally:
        dev.close()
        fresh.close()


LIT_LIGHT_TO = dict(corner=(-0.2, 2.0, -1.0), edgeU=(0.0, 0.3, 1.4), edgeV=(1.8, 0.2, 0.0), normal=(0.0, -1.0, 0.1))


@pytest.mark.parametrize("metal", [0, pt.PTR_METAL_FACE_NORMAL | pt.PTR_METAL_SPECULAR | pt.PTR_METAL_CLAMPS], ids=["default", "metal"])
def test_render_with_a_moved_light_equals_a_fresh_uploads(hosts, metal):
    """Scene A's walls meet in shared edges, where a refitted and a fresh tree may settle tied hits differently; its own test follows.
    Here the light moves twice in the tie-free soup under a light, where no hit can tie."""
    host = hosts("lit")
    s = small_settings(host, 64, 48, 4, metal)
    dev = upload(host)
    fresh = upload(dsc.Changed(host, rects={0: pt.rect_update(0, **LIT_LIGHT_TO)}), dynamic=False)
    try:
        before = dev.render_image(s, 4)[0]
        dev.set_rects({0: dict(corner=(0.5, 3.0, 0.0), edgeU=(1.0, 0.0, 0.0), edgeV=(0.0, 0.0, 1.0), normal=(0.0, -1.0, 0.0))})
        dev.set_rects({0: LIT_LIGHT_TO})
        got = dev.render_image(s, 4)[0]
        assert_same_image(got, fresh.render_image(s, 4)[0], "the lit soup with its light moved")
        assert not np.array_equal(got, before)
    finally:
        dev.close()
        fresh.close()


def test_render_of_scene_a_with_its_light_moved_equals_a_fresh_uploads(hosts):
    host = hosts("A")
    s = small_settings(host, 64, 48, 4)
    dev, fresh = upload(host), upload(dsc.Changed(host, rects={LIGHT: pt.rect_update(LIGHT, **LIGHT_TO)}), dynamic=False)
    try:
        dev.set_rects({LIGHT: LIGHT_TO})
        assert_same_image(dev.render_image(s, 4)[0], fresh.render_image(s, 4)[0], "scene A with its light moved")
    finally:
        dev.close()
        fresh.close()


def test_frame_after_an_update(hosts):
    host = hosts("lit")
    dev = upload(host)
    try:
        s = small_settings(host)
        frame = dev.frame(s)
        frame.accumulate(2)
        stale = frame.resolve()[0]
        dev.set_mesh_vertices({1: waved(host, 1, 0.8)})
        dev.set_rects({0: LIT_LIGHT_TO})
        frame.reset()
        frame.accumulate(4)
        rgb, _, count = frame.resolve()
        want = dev.render_image(s, 4)[0]
        assert (count == 4).all() and np.array_equal(rgb, want) and not np.array_equal(stale, want)
        frame.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 6. background cull
def test_world_bounds_follow_a_sphere_moved_far_outside(hosts):
    host = hosts("lit")
    to = (0.5, 4.5, 0.3, 0.6)   # two units above the light, the top of the old bounds
    s = small_settings(host, 64, 48, 4)
    s.cameraVerticalFov = 90.0   # wide enough to see it there
    dev, fresh = upload(host), upload(dsc.Changed(host, spheres={0: to}), dynamic=False)
    try:
        base = dev.render_image(s, 4)[0]
        old_hi = np.array(dev.set_spheres({0: list(host.desc.spheres[0].centerRadius)})["sceneHi"])
        info = dev.set_spheres({0: to})
        assert info["sceneHi"][1] > old_hi[1] + 2.0
        got, want = dev.render_image(s, 4)[0], fresh.render_image(s, 4)[0]
        assert_same_image(got, want, "the lit soup with its sphere far above")
        # the sphere shows against the sky, where the old bounds had nothing to hit: the image changed near its top or bottom edge
        diff = (got != base).any(axis=2)
        assert diff[:12].any() or diff[-12:].any()
    finally:
        dev.close()
        fresh.close()


# --------------------------------------------------------------------------------------------------------------------- 7. refusals
def test_what_the_updates_refuse(hosts):
    host = hosts("textured")
    dev = upload(host)
    lib = pt.load_library()
    err = C.create_string_buffer(512)
    fp = C.POINTER(C.c_float)
    try:
        before = dev.arrays()
        pos, nrm, tan = dsc.original(host, 0)
        n = len(pos)

        def vertices(items, count=None, pointer=True):
            arr = (pt.PtrMeshVertices * max(len(items), 1))()
            keep = []
            for k, (index, vc, p, q, t) in enumerate(items):
                arr[k].meshIndex, arr[k].vertexCount = index, vc
                for name, a in (("positions", p), ("normals", q), ("tangents", t)):
                    if a is not None:
                        a = np.ascontiguousarray(a, np.float32)
                        keep.append(a)
                        setattr(arr[k], name, a.ctypes.data_as(fp))
            rc = lib.ptr_scene_set_mesh_vertices(dev._h, arr if pointer else None, len(items) if count is None else count, None, None, err, len(err))
            return rc, err.value.decode()

        def poisoned(a, value):
            b = a.copy()
            b[n // 2, 1] = value
            return b

        good = (0, n, pos, nrm, tan)
        cases = [("null list", vertices([], 1, False), "null"), ("count 0", vertices([good], 0), "count is 0"),
                 ("index out of range", vertices([(host.desc.meshCount, n, pos, nrm, tan)]), "out of range"),
                 ("index named twice", vertices([good, good]), "named twice"),
                 ("vertex count", vertices([(0, n - 1, pos[:-1], nrm[:-1], tan[:-1])]), "vertices"),
                 ("null positions", vertices([(0, n, None, nrm, tan)]), "null positions"), ("null normals", vertices([(0, n, pos, None, tan)]), "null normals"),
                 ("tangents missing", vertices([(0, n, pos, nrm, None)]), "with tangents"),
                 ("NaN position", vertices([(0, n, poisoned(pos, np.nan), nrm, tan)]), "non-finite position"),
                 ("infinite normal", vertices([(0, n, pos, poisoned(nrm, np.inf), tan)]), "non-finite normal"),
                 ("NaN tangent", vertices([(0, n, pos, nrm, poisoned(tan, np.nan))]), "non-finite tangent")]
        for name, (rc, message), pattern in cases:
            assert rc != 0 and message.startswith("ptr_scene_set_mesh_vertices:") and re.search(pattern, message), (name, rc, message)
        same_arrays(dev.arrays(), before, "after the refused ptr_scene_set_mesh_vertices calls")

        good_rect = dict(corner=(0.0, 5.0, 0.0), edgeU=(1.0, 0.0, 0.0), edgeV=(0.0, 0.0, 1.0), normal=(0.0, -1.0, 0.0))

        def rects(items, count=None, pointer=True):
            arr = (pt.PtrRectUpdate * max(len(items), 1))(*items)
            rc = lib.ptr_scene_set_rects(dev._h, arr if pointer else None, len(items) if count is None else count, None, None, err, len(err))
            return rc, err.value.decode()

        nan_rect, flat_rect, no_normal = pt.rect_update(0, **good_rect), pt.rect_update(0, **dict(good_rect, edgeV=(-3.0, 0.0, 0.0))), pt.rect_update(0, **good_rect)
        nan_rect.edgeU[3] = float("nan")
        no_normal.normalAndPlane[:] = [0.0, 0.0, 0.0, 1.0]
        ok = pt.rect_update(0, **good_rect)
        cases = [("null list", rects([], 1, False), "null"), ("count 0", rects([ok], 0), "count is 0"),
                 ("index out of range", rects([pt.rect_update(host.desc.rectCount, **good_rect)]), "out of range"),
                 ("index named twice", rects([ok, ok]), "named twice"), ("NaN entry", rects([nan_rect]), "non-finite"),
                 ("parallel edges", rects([flat_rect]), "cross"), ("zero normal", rects([no_normal]), "normal of length zero")]
        for name, (rc, message), pattern in cases:
            assert rc != 0 and message.startswith("ptr_scene_set_rects:") and re.search(pattern, message), (name, rc, message)
        same_arrays(dev.arrays(), before, "after the refused ptr_scene_set_rects calls")
    finally:
        dev.close()
    # tangents for a mesh uploaded without them, and what ptr_scene_set_spheres refuses, on scene A
    host = hosts("A")
    dev = upload(host)
    try:
        before = dev.arrays()
        pos, nrm = dsc.original(host, 0)
        with pytest.raises(pt.PtrError, match="ptr_scene_set_mesh_vertices: .*without tangents"):
            dev.set_mesh_vertices({0: (pos, nrm, np.ones((len(pos), 4), np.float32))})

        def spheres(items, count=None, pointer=True):
            arr = (pt.PtrSphereUpdate * max(len(items), 1))()
            for k, (index, row) in enumerate(items):
                arr[k].sphereIndex = index
                arr[k].centerRadius[:] = row
            rc = lib.ptr_scene_set_spheres(dev._h, arr if pointer else None, len(items) if count is None else count, None, None, err, len(err))
            return rc, err.value.decode()

        row = [1.0, 2.0, 3.0, 4.0]
        cases = [("null list", spheres([], 1, False), "null"), ("count 0", spheres([(0, row)], 0), "count is 0"),
                 ("index out of range", spheres([(host.desc.sphereCount, row)]), "out of range"), ("index named twice", spheres([(0, row), (0, row)]), "named twice"),
                 ("NaN radius", spheres([(0, [1.0, 2.0, 3.0, float("nan")])]), "non-finite")]
        for name, (rc, message), pattern in cases:
            assert rc != 0 and message.startswith("ptr_scene_set_spheres:") and re.search(pattern, message), (name, rc, message)
        same_arrays(dev.arrays(), before, "after the refused calls on scene A")
    finally:
        dev.close()


def test_a_mesh_without_triangles_is_accepted(hosts):
    host = hosts("F-triangle")
    bare = dsc.Changed(host)
    bare._meshes[0].indexCount = 0
    dev = upload(bare)
    try:
        before = dev.arrays()
        info = dev.set_mesh_vertices({0: dsc.displaced(host)})
        assert (info["trianglesMoved"], info["nodes"]) == (0, 0)
        same_arrays(dev.arrays(), before, "a mesh without triangles")
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 8. flags
def test_flags(hosts):
    host = hosts("A")
    plain, ex0 = upload(host, deformable=False, primitives=False), None
    lib = pt.load_library()
    err = C.create_string_buffer(512)
    h = C.c_void_p()
    assert lib.ptr_scene_upload_dynamic_ex(C.byref(host.desc), 0, 0, C.byref(h), err, len(err)) == 0, err.value
    try:
        assert plain.is_dynamic and plain.dynamic_flags == 0 and lib.ptr_scene_is_dynamic(h) == 1 and lib.ptr_scene_dynamic_flags(h) == 0
        size_a, size_b = C.c_uint64(0), C.c_uint64(0)
        for name, (which, _, _) in pt.SCENE_ARRAYS.items():
            assert lib.ptr_debug_scene_arrays(plain._h, which, None, 0, C.byref(size_a)) == 0 and lib.ptr_debug_scene_arrays(h, which, None, 0, C.byref(size_b)) == 0
            assert size_a.value == size_b.value, name
        before = plain.arrays()
        pos, nrm = dsc.original(host, 0)
        with pytest.raises(pt.PtrError, match="ptr_scene_set_mesh_vertices: the scene is not deformable"):
            plain.set_mesh_vertices({0: (pos, nrm)})
        with pytest.raises(pt.PtrError, match="ptr_scene_set_spheres: the scene does not keep its primitives"):
            plain.set_spheres({0: SPHERE_TO})
        with pytest.raises(pt.PtrError, match="ptr_scene_set_rects: the scene does not keep its primitives"):
            plain.set_rects({LIGHT: LIGHT_TO})
        same_arrays(plain.arrays(), before, "after the refused calls")
        # each flag opens its own calls only
        for deformable, primitives in ((True, False), (False, True)):
            dev = upload(host, deformable=deformable, primitives=primitives)
            try:
                assert dev.dynamic_flags == (1 if deformable else 2)
                if deformable:
                    dev.set_mesh_vertices({0: (pos, nrm)})
                    with pytest.raises(pt.PtrError, match="does not keep its primitives"):
                        dev.set_spheres({0: SPHERE_TO})
                else:
                    dev.set_spheres({0: SPHERE_TO})
                    with pytest.raises(pt.PtrError, match="not deformable"):
                        dev.set_mesh_vertices({0: (pos, nrm)})
            finally:
                dev.close()
        static = upload(host, dynamic=False)
        try:
            with pytest.raises(pt.PtrError, match="not deformable"):
                static.set_mesh_vertices({0: (pos, nrm)})
        finally:
            static.close()
    finally:
        plain.close()
        lib.ptr_scene_release(h)
