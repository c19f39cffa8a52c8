"""Dynamic scenes on the device (include/ptr_dynamic.h): ptr_scene_set_mesh_transforms against what a fresh upload of the moved
description produces.  Every comparison of arrays and images is exact (bit patterns); the ray-by-ray comparisons with the oracle use
check_extend of test_gpu_traversal.py with that file's own thresholds."""
import ctypes as C
import os

import numpy as np
import pytest

import dynamic_ref as dr
import oracle_lib as ol
import traversal_ref as tr
import traversal_scenes as ts
from test_gpu_traversal import check_extend, knobs, oracle, _first

pt = ts.pt
pytestmark = pytest.mark.gpu

GOLDEN = ts.GOLDEN
FORMATS = [("default", {}), ("PTR_WIDE_NODES=0", {"PTR_WIDE_NODES": "0"}), ("PTR_QUANTIZED_NODES=0", {"PTR_QUANTIZED_NODES": "0"})]
FORMAT_IDS = [f[0] for f in FORMATS]


# --------------------------------------------------------------------------------------------------------------------- descriptions
class Moved:
    """A copy of a host scene's description whose meshes carry other localToWorld matrices ({mesh index: 4x4 float32, row / column})."""

    def __init__(self, host, matrices):
        self._host = host
        d = host.desc
        self._meshes = (pt.PtrMeshDesc * max(d.meshCount, 1))()
        for i in range(d.meshCount):
            C.memmove(C.byref(self._meshes[i]), C.byref(d.meshes[i]), C.sizeof(pt.PtrMeshDesc))
        for i, m in matrices.items():
            self._meshes[i].localToWorld[:] = np.asarray(m, np.float32).T.reshape(-1).tolist()
        self.desc = pt.PtrSceneDesc()
        C.memmove(C.byref(self.desc), C.byref(d), C.sizeof(pt.PtrSceneDesc))
        self.desc.meshes = C.cast(self._meshes, C.POINTER(pt.PtrMeshDesc))

    def settings_for(self, **kw):
        return self._host.settings_for(**kw)


def matrix_of(host, mesh=0):
    return np.array(list(host.desc.meshes[mesh].localToWorld), np.float32).reshape(4, 4).T.copy()


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.eye(4)
    r[:3, :3] = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    return r


def compose(translate, rot, scale):
    t, s = np.eye(4), np.diag([scale[0], scale[1], scale[2], 1.0])
    t[:3, 3] = translate
    return t @ rot @ s


def t1_t2(host, mesh=0):
    """T1: rotation about a skew axis x non-uniform scale x a translation several scene boxes long, on top of the mesh's matrix;
    T2: T1 with the x axis mirrored first.  float32, the values both the update and the moved description get."""
    lo, hi = ts.bounds(tr.Reference(host.desc))
    shift = 3.0 * float(np.max(hi - lo)) * np.array([1.0, 0.5, -0.7])
    base = matrix_of(host, mesh).astype(np.float64)
    t1 = compose(shift, rotation((0.3, 1.0, -0.45), 0.7), (1.3, 0.7, 1.1))
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0])
    return (t1 @ base).astype(np.float32), (t1 @ mirror @ base).astype(np.float32)


def upload(desc_holder, env=None, dynamic=True):
    with knobs(env or {}):
        return pt.DeviceScene(desc_holder.desc, 0, keepalive=desc_holder, dynamic=dynamic)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    cache = {}

    def get(key):
        if key not in cache:
            tmp = tmp_path_factory.mktemp("dyn_" + key.replace("-", "_"))
            if key == "textured":
                cache[key] = pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN)
            elif key in ("A", "C"):
                cache[key] = ts.scene_a() if key == "A" else ts.scene_c()
            elif key == "D":
                cache[key] = ts.scene_d(tmp)
            elif key == "E":
                cache[key] = ts.scene_e(tmp, count=20000)
            elif key == "soup":
                cache[key] = soup_scene(tmp)
            else:
                cache[key] = ts.scene_f(tmp, key[2:])
        return cache[key]
    return get


def same_arrays(got, want, what, names=None):
    for name in (names or want):
        assert got[name].shape == want[name].shape and np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), \
            "%s: array %s differs in %d words" % (what, name, int((got[name].view(np.uint32) != want[name].view(np.uint32)).sum())
                                                  if got[name].shape == want[name].shape else -1)


def small_settings(holder, width=32, height=24, depth=4, metal=0):
    s = holder.settings_for(width=width, height=height, max_depth=depth, seed=1337)
    s.metalSemantics = metal
    return s


# --------------------------------------------------------------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("key", ["A", "D", "textured", "F-triangle", "F-coincident"])
def test_round_trip_restores_every_array(hosts, key, fmt):
    host = hosts(key)
    dev = upload(host, fmt[1])
    try:
        assert dev.is_dynamic
        first = dev.arrays()
        s = small_settings(host)
        before = dev.render_image(s, 4)[0]
        t1, _ = t1_t2(host)
        dev.set_mesh_transforms({0: t1})
        moved = dev.arrays()
        assert not np.array_equal(moved["tris"], first["tris"]) and not np.array_equal(moved["grid"], first["grid"])
        assert not np.array_equal(moved["triBounds"], first["triBounds"]) and not np.array_equal(moved["boxes"], first["boxes"])
        dev.set_mesh_transforms({0: matrix_of(host)})
        same_arrays(dev.arrays(), first, "scene %s, %s, after the round trip" % (key, fmt[0]))
        assert np.array_equal(dev.render_image(s, 4)[0], before)
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 2. fresh upload
def by_meta(a):
    """Order of the triangles by their meta words (kind | class | geometry, primitive index)."""
    w = a["tris"].view(np.uint32)
    key = (w[:, 1, 3].astype(np.uint64) << np.uint64(32)) | w[:, 2, 3].astype(np.uint64)
    assert len(np.unique(key)) == len(key)
    return np.argsort(key)


@pytest.mark.parametrize("which", ["T1", "T2"])
@pytest.mark.parametrize("key", ["A", "D", "textured"])
def test_moved_arrays_equal_a_fresh_uploads(hosts, key, which):
    host = hosts(key)
    m = t1_t2(host)[0 if which == "T1" else 1]
    dev, fresh = upload(host), upload(Moved(host, {0: m}))
    try:
        info = dev.set_mesh_transforms({0: m})
        got, want = dev.arrays(), fresh.arrays()
        go, wo = by_meta(got), by_meta(want)
        what = "scene %s, %s" % (key, which)
        for name in ("tris", "triNormals", "triUv", "triTangent", "triBounds"):
            assert len(got[name]) == len(want[name]), (what, name)
            if len(got[name]):
                a, b = got[name][go].view(np.uint32), want[name][wo].view(np.uint32)
                assert np.array_equal(a, b), "%s: %s differs on %d triangles, first %s" % (what, name, int((a != b).any(axis=(1, 2)).sum()),
                                                                                           np.flatnonzero((a != b).any(axis=(1, 2)))[:4])
        if key == "textured":
            assert len(got["triUv"]) and len(got["triTangent"])
        # the tree: boxes from the downloaded bounds, the grid from the root box, the quantised and the wide nodes from the boxes
        t = pt.debug_dynamic_tables(host.desc, ["schedule", "levelOffsets", "wideSource"])
        boxes = dr.refit(got["boxes"], t["schedule"], t["levelOffsets"], got["triBounds"], got["sphereBounds"])
        same_arrays({"boxes": got["boxes"]}, {"boxes": boxes}, what + " (refit reference)")
        lo, hi = dr.root_box(got["boxes"])
        grid = dr.grid_of(lo, hi)
        same_arrays({"grid": got["grid"]}, {"grid": grid}, what)
        assert np.array_equal(np.array(info["sceneLo"], np.float32), lo) and np.array_equal(np.array(info["sceneHi"], np.float32), hi)
        q = dr.quantise(got["boxes"], grid)
        assert len(got["qnodes"]) and np.array_equal(got["qnodes"], q), what
        assert len(got["wnodes"]) and np.array_equal(got["wnodes"], dr.wide_copy(got["wnodes"], q, t["wideSource"])), what
    finally:
        dev.close()
        fresh.close()


# --------------------------------------------------------------------------------------------------------------------- 3. hits
@pytest.mark.parametrize("key", ["A", "C", "D", "E"])
def test_hits_after_an_update_equal_the_oracles(hosts, key):
    host = hosts(key)
    m = t1_t2(host)[0]
    moved = Moved(host, {0: m})
    ref, osc = tr.Reference(moved.desc), ol.OracleScene(moved)
    rays, edge = ts.mixed_rays(ref, 20000, 707, ties=True)
    o = oracle(osc, rays)
    any_rays = rays[:6000]
    want_any = oracle(osc, any_rays, any_hit=True)["t"] >= 0
    assert (o["t"] >= 0).any()
    for fname, env in FORMATS:
        dev = upload(host, env)
        try:
            dev.set_mesh_transforms({0: m})
            for count in ((False, True) if fname == "default" else (False,)):
                g, info = dev.extend_rays(rays, count=count)
                where = "scene %s moved, node format %s (launched %s)" % (key, fname, pt.DeviceScene.NODE_FORMATS[info["format"]])
                check_extend(where, rays, g, o, aimed_at_edges=edge)
            c, _ = dev.trace_rays(rays)
            check_extend("scene %s moved, %s, ptr_trace_rays" % (key, fname), rays, c, o, aimed_at_edges=edge)
            occ, info = dev.connect_rays(any_rays, records_per_slot=2)
            assert np.array_equal(occ, want_any), "scene %s moved, %s: %d rays occluded differently: %s" % (
                key, fname, int((occ != want_any).sum()), _first(any_rays, occ != want_any, ("gpu", occ), ("oracle", want_any)))
        finally:
            dev.close()


# --------------------------------------------------------------------------------------------------------------------- 4. render
def soup_scene(tmp):
    """Two meshes, each 1500 small triangles, one per cell of a jittered 12 x 12 x 11 grid with margins: no shared edge or vertex, no
    rectangle, so no two hits tie.  Object space spans +-0.6; the meshes sit at x = -2 and x = +2."""
    rng = np.random.default_rng(11)
    for name in ("soup_a", "soup_b"):
        cells = rng.permutation(12 * 12 * 11)[:1500]
        c = np.stack([cells % 12, (cells // 12) % 12, cells // 144], axis=1) * 0.1 + 0.05 - np.array([0.6, 0.6, 0.55])
        v = c[:, None, :] + rng.uniform(-0.035, 0.035, (1500, 3, 3))
        with open(tmp / (name + ".obj"), "w") as f:
            f.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in v.reshape(-1, 3))
            f.writelines("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3) for k in range(1500))
    p = tmp / "soup.scene"
    p.write_text("camera target=0,0,0 distance=7 yaw=1.5708 pitch=0.2 vfov=40\nrenderer maxDepth=4 seed=1337\nbackground\n"
                 "material type=lambert albedo=0.7,0.5,0.3\nmaterial type=metal albedo=0.8,0.8,0.9 fuzz=0.1\n"
                 "mesh path=soup_a.obj translate=-2,0,0 material=0\nmesh path=soup_b.obj translate=2,0,0 material=1\n")
    return ts.load(p, str(tmp))


def soup_pose(host, angle, axis, scale, offset):
    base = matrix_of(host, 1).astype(np.float64)   # a translation to (2, 0, 0): the pose turns the mesh about its own centre
    return (base @ compose(offset, rotation(axis, angle), scale)).astype(np.float32)


@pytest.mark.parametrize("metal", [0, pt.PTR_METAL_FACE_NORMAL | pt.PTR_METAL_SPECULAR | pt.PTR_METAL_CLAMPS], ids=["default", "metal"])
def test_render_equals_a_fresh_uploads(hosts, metal):
    host = hosts("soup")
    assert host.desc.meshCount == 2 and host.desc.rectCount == 0
    poses = [soup_pose(host, 0.4, (1, 0.2, 0), (1.0, 1.0, 1.0), (0.1, 0, 0)), soup_pose(host, 2.1, (0.1, 1, 0.3), (1.2, 0.8, 1.0), (0, 0.2, -0.1)),
             soup_pose(host, -1.3, (0.5, -0.4, 1), (-0.9, 1.1, 1.25), (0.15, -0.1, 0.2))]
    s = small_settings(host, 64, 48, 4, metal)
    dev, fresh = upload(host), upload(Moved(host, {1: poses[2]}), dynamic=False)
    try:
        for pose in poses:
            dev.set_mesh_transforms({1: pose})
        got, want = dev.render_image(s, 4)[0], fresh.render_image(s, 4)[0]
        assert want.max() > 0 and np.isfinite(want).all()
        diff = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2)
        if diff.any():
            _, sig_got = dev.render_signatures(s)
            _, sig_want = fresh.render_signatures(s)
            ys, xs = np.nonzero(diff)
            pytest.fail("%d pixels differ; (x, y, updated rgb, fresh rgb, 1-spp signature updated / fresh): %s" % (
                int(diff.sum()), [(int(x), int(y), got[y, x].tolist(), want[y, x].tolist(), hex(int(sig_got[y, x])), hex(int(sig_want[y, x])))
                                  for y, x in list(zip(ys, xs))[:6]]))
    finally:
        dev.close()
        fresh.close()


# --------------------------------------------------------------------------------------------------------------------- 5. frames
def test_frame_after_an_update(hosts):
    host = hosts("A")
    dev = upload(host)
    try:
        s = small_settings(host)
        frame = dev.frame(s)
        frame.accumulate(2)
        stale = frame.resolve()[0]
        dev.set_mesh_transforms({0: t1_t2(host)[0]})
        frame.reset()
        frame.accumulate(4)
        rgb, _, count = frame.resolve()
        want = dev.render_image(s, 4)[0]
        assert (count == 4).all() and np.array_equal(rgb, want) and not np.array_equal(stale, want)
        frame.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 6. refusals
def test_what_an_update_refuses(hosts):
    host = hosts("A")
    dev, plain = upload(host), upload(host, dynamic=False)
    try:
        assert dev.is_dynamic and not plain.is_dynamic
        with pytest.raises(pt.PtrError, match="dynamic"):
            plain.set_mesh_transforms({0: np.eye(4)})
        before = dev.arrays()
        good = matrix_of(host)
        lib = pt.load_library()
        err = C.create_string_buffer(512)

        def call(items, count, pointer=True):
            arr = (pt.PtrMeshTransform * max(len(items), 1))()
            for k, (index, m) in enumerate(items):
                arr[k].meshIndex = index
                arr[k].localToWorld[:] = np.asarray(m, np.float32).T.reshape(-1).tolist()
            rc = lib.ptr_scene_set_mesh_transforms(dev._h, arr if pointer else None, count, None, None, err, len(err))
            return rc, err.value.decode()

        nan, inf, flat, tiny = good.copy(), good.copy(), good.copy(), good.copy()
        nan[1, 2] = np.nan
        inf[0, 3] = np.inf
        flat[:3, 2] = flat[:3, 1]                    # two equal columns: determinant 0
        tiny[:3, :3] = np.eye(3) * np.float32(1e-30)  # determinant underflows to 0 / the inverse overflows
        cases = [("null list", ([], 1, False), "null"), ("count 0", ([(0, good)], 0), "count is 0"),
                 ("index out of range", ([(host.desc.meshCount, good)], 1), "out of range"),
                 ("index named twice", ([(0, good), (0, good)], 2), "named twice"), ("NaN entry", ([(0, nan)], 1), "non-finite"),
                 ("infinite entry", ([(0, inf)], 1), "non-finite"), ("singular matrix", ([(0, flat)], 1), "determinant"),
                 ("degenerate scale", ([(0, tiny)], 1), "determinant|not finite")]
        import re
        for name, args, pattern in cases:
            rc, message = call(*args)
            assert rc != 0 and message.startswith("ptr_scene_set_mesh_transforms:") and re.search(pattern, message), (name, rc, message)
            same_arrays(dev.arrays(), before, "after the refused call (%s)" % name)
    finally:
        dev.close()
        plain.close()


def test_a_mesh_without_triangles_on_a_tree_without_nodes(hosts):
    host = hosts("F-triangle")
    bare = Moved(host, {})
    bare._meshes[0].indexCount = 0          # the scene's only primitive is gone: no node, no level
    dev = upload(bare)
    try:
        before = dev.arrays()
        assert len(before["tris"]) == 0 and len(before["boxes"]) == 0 and len(before["qnodes"]) == 0
        info = dev.set_mesh_transforms({0: t1_t2(host)[0]})
        assert (info["trianglesMoved"], info["nodes"], info["levels"], info["wideNodes"]) == (0, 0, 0, 0)
        same_arrays(dev.arrays(), before, "a mesh without triangles")
        assert np.isfinite(dev.render_image(small_settings(host), 1)[0]).all()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 7. info
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_update_info(hosts, fmt):
    host = hosts("A")
    dev = upload(host, fmt[1])
    try:
        with knobs(fmt[1]):
            t = pt.debug_dynamic_tables(host.desc, ["info", "meshTriOffsets"])
        info = dev.set_mesh_transforms({0: t1_t2(host)[0]})
        a = dev.arrays(["boxes", "grid"])
        assert info["trianglesMoved"] == int(t["meshTriOffsets"][1] - t["meshTriOffsets"][0]) == host.desc.meshes[0].indexCount // 3
        assert (info["nodes"], info["levels"], info["wideNodes"]) == (t["info"]["nodes"], t["info"]["levels"], t["info"]["wide_nodes"])
        lo, hi = dr.root_box(a["boxes"])
        assert np.array_equal(np.array(info["sceneLo"], np.float32), lo) and np.array_equal(np.array(info["sceneHi"], np.float32), hi)
        assert np.array_equal(np.array([info["gridOrigin"], info["gridCell"]], np.float32), a["grid"])
        assert info["totalSeconds"] > 0 and min(info["bakeMs"], info["refitMs"], info["quantiseMs"], info["wideMs"]) >= 0 and info["cellOverExtent"] > 0
    finally:
        dev.close()
