"""The rebuild above the leaves on the device (include/ptr_rebuild.h): ptr_scene_rebuild_tree against the numpy reference tree
(rebuild_ref.py) and the builder's own functions (ptr_debug_rebuild_tables), and ptr_scene_tree_cost against float64 numpy.  Every
comparison of arrays and images is exact (bit patterns); the ray-by-ray comparisons with the oracle use check_extend of
test_gpu_traversal.py with that file's own thresholds; tree_cost is held to a relative 1e-9 (double rounding times the at most 10^6 terms
of these scenes)."""
import ctypes as C

import numpy as np
import pytest

import deform_scenes as dsc
import dynamic_ref as dr
import oracle_lib as ol
import rebuild_ref as rr
import rebuild_scenes as rs
import traversal_ref as tr
import traversal_scenes as ts
from test_gpu_traversal import check_extend, knobs, oracle, _first

pt = ts.pt
pytestmark = pytest.mark.gpu

FORMATS = [("default", {}), ("PTR_WIDE_NODES=0", {"PTR_WIDE_NODES": "0"}), ("PTR_QUANTIZED_NODES=0", {"PTR_QUANTIZED_NODES": "0"})]
FORMAT_IDS = [f[0] for f in FORMATS]
LEAF_ORDER = ("tris", "triNormals", "triUv", "triTangent", "triBounds", "sphereBounds", "spheres", "rects", "rectLights", "objPos", "objNrm", "objTan")
METAL = pt.PTR_METAL_FACE_NORMAL | pt.PTR_METAL_SPECULAR | pt.PTR_METAL_CLAMPS


class Moved:
    """A copy of a host scene's description whose meshes carry other localToWorld matrices ({mesh index: 4x4 float32, row / column})."""

    def __init__(self, host, matrices):
        self._inner = dsc.Changed(host, matrices=matrices)
        self.desc = self._inner.desc

    def settings_for(self, **kw):
        return self._inner.settings_for(**kw)


def matrix_of(host, mesh=0):
    return np.array(list(host.desc.meshes[mesh].localToWorld), np.float32).reshape(4, 4).T.copy()


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.eye(4)
    r[:3, :3] = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    return r


def turned(host, mesh=0, angle=0.7):
    """The mesh turned about a skew axis through its own origin and scaled unevenly: the refitted boxes of its subtree loosen."""
    s = np.diag([1.3, 0.7, 1.1, 1.0])
    return (matrix_of(host, mesh).astype(np.float64) @ rotation((0.3, 1.0, -0.45), angle) @ s).astype(np.float32)


def upload(holder, env=None, dynamic=True, **kw):
    with knobs(env or {}):
        return pt.DeviceScene(holder.desc, 0, keepalive=holder, dynamic=dynamic, **kw)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = rs.host_scene(key, tmp_path_factory.mktemp("rbg_" + key.replace("-", "_")))
        return cache[key]
    return get


def same_arrays(got, want, what, names=None):
    for name in (names or want):
        assert got[name].shape == want[name].shape and np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), \
            "%s: array %s differs in %d words" % (what, name, int((got[name].view(np.uint32) != want[name].view(np.uint32)).sum())
                                                  if got[name].shape == want[name].shape else -1)


def everything(dev):
    out = dev.arrays()
    out.update({"rb_" + k: v for k, v in dev.rebuild_arrays(["schedule", "levelOffsets", "wideSource", "pointers"]).items()})
    return out


def small_settings(holder, width=32, height=24, depth=4, metal=0):
    s = holder.settings_for(width=width, height=height, max_depth=depth, seed=1337)
    s.metalSemantics = metal
    return s


def check_tree(dev, what, collapsed_now=True):
    """The scene's node arrays against dynamic_ref and the builder's functions on its own float nodes and bounds, whatever the topology.
    collapsed_now: the four-wide nodes were chosen on these boxes (right after a rebuild); an update keeps the choice and copies boxes."""
    got, rb = dev.arrays(), dev.rebuild_arrays()
    boxes = dr.refit(got["boxes"], rb["schedule"], rb["levelOffsets"], got["triBounds"], got["sphereBounds"])
    same_arrays({"boxes": got["boxes"]}, {"boxes": boxes}, what + " (refit reference)")
    probe = pt.debug_rebuild_tables(got["boxes"])
    assert np.array_equal(rb["schedule"], probe["schedule"]) and np.array_equal(rb["levelOffsets"], probe["levelOffsets"]), what
    same_arrays({"grid": got["grid"]}, {"grid": probe["grid"]}, what)
    if len(got["qnodes"]):
        assert np.array_equal(got["qnodes"], probe["qnodes"]) and np.array_equal(got["qnodes"], dr.quantise(got["boxes"], got["grid"])), what
    if len(got["wnodes"]):
        assert np.array_equal(got["wnodes"], dr.wide_copy(got["wnodes"], got["qnodes"], rb["wideSource"])), what
        used = rb["wideSource"] != dr.NO_SOURCE
        assert np.array_equal(got["wnodes"][~used], np.broadcast_to(np.array([0xFFFFFFFF, 0xFFFF, 0, dr.EMPTY], np.uint32), got["wnodes"][~used].shape)), what
    if len(got["wnodes"]) and collapsed_now:
        assert np.array_equal(got["wnodes"], probe["wnodes"]) and np.array_equal(rb["wideSource"], probe["wideSource"]), what
        assert rb["info"]["wide_depth"] == probe["wideDepth"] and rb["info"]["wide_nodes"] == len(probe["wnodes"]), what
    assert rb["info"]["levels"] == len(probe["levelOffsets"]) - 1 and rb["info"]["stack_limit"] >= 16
    return got, rb, probe


# --------------------------------------------------------------------------------------------------------------------- 1. arrays
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("key", ["A", "C", "D", "textured", "F-coincident", "strip", "E", "soup"])
def test_arrays_after_a_rebuild(hosts, key, fmt):
    host = hosts(key)
    dev = upload(host, fmt[1])
    try:
        what = "scene %s, %s" % (key, fmt[0])
        if host.desc.meshCount and key != "F-coincident":
            dev.set_mesh_transforms({0: turned(host)})
        moved = dev.arrays()
        cost_moved = dev.tree_cost()
        assert np.isclose(cost_moved, rr.tree_cost(moved["boxes"]), rtol=1e-9, atol=0), what
        want, schedule, offsets = rs.reference_tree(moved["boxes"], moved["triBounds"], moved["sphereBounds"])
        info = dev.rebuild_tree(keep_if_better=False)
        got, rb, probe = check_tree(dev, what)
        assert np.array_equal(dr.refs_of(got["boxes"]), dr.refs_of(want)), what + ": topology"
        same_arrays({"boxes": got["boxes"]}, {"boxes": want}, what)
        assert np.array_equal(rb["schedule"], schedule) and np.array_equal(rb["levelOffsets"], offsets)
        same_arrays(got, moved, what + " (untouched)", LEAF_ORDER + ("grid",))
        assert info["installed"] == 1 and info["nodes"] == len(want) and info["levels"] == len(offsets) - 1 and info["leaves"] == len(want) + 1
        assert info["wideNodes"] == len(got["wnodes"]) and info["wideDepth"] == (probe["wideDepth"] if len(got["wnodes"]) else 0)
        assert info["costBefore"] == cost_moved and info["costAfter"] == dev.tree_cost()
        assert np.isclose(info["costAfter"], rr.tree_cost(got["boxes"]), rtol=1e-9, atol=0), what
        assert info["totalSeconds"] > 0 and info["keysSortMs"] > 0 and info["topologyMs"] > 0 and info["fitMs"] > 0
    finally:
        dev.close()


def test_tree_cost_of_a_fresh_upload_is_the_builders(hosts):
    for key in ("A", "D", "F-triangle", "F-coincident"):
        dev = upload(hosts(key))
        try:
            cost = dev.tree_cost()
            assert int(cost * 1000.0) == dev.info()["sah_cost_x1000"], key
            assert cost == dev.tree_cost()
        finally:
            dev.close()


# --------------------------------------------------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("key", ["A", "soup"])
def test_a_rebuild_is_a_function_of_the_geometry(hosts, key, fmt):
    host = hosts(key)
    mesh = host.desc.meshCount - 1
    one, two = upload(host, fmt[1]), upload(host, fmt[1])
    try:
        one.set_mesh_transforms({mesh: turned(host, mesh)})
        one.rebuild_tree(keep_if_better=False)
        first = everything(one)
        one.rebuild_tree(keep_if_better=False)   # built into the other set of arrays
        again = everything(one)
        names = [n for n in first if n != "rb_pointers"]
        same_arrays(again, first, "rebuilt twice", names)
        assert not np.array_equal(again["rb_pointers"], first["rb_pointers"])
        two.rebuild_tree(keep_if_better=False)
        two.set_mesh_transforms({mesh: turned(host, mesh)})
        two.rebuild_tree(keep_if_better=False)
        same_arrays(everything(two), first, "upload, rebuild, move, rebuild", names)
    finally:
        one.close()
        two.close()


# --------------------------------------------------------------------------------------------------------------------- 3. hits
@pytest.mark.parametrize("key", ["A", "C", "D", "E"])
def test_hits_after_a_rebuild_equal_the_oracles(hosts, key):
    host = hosts(key)
    m = turned(host)
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
            assert dev.rebuild_tree(keep_if_better=False)["installed"] == 1
            for count in ((False, True) if fname == "default" else (False,)):
                g, info = dev.extend_rays(rays, count=count)
                where = "scene %s rebuilt, node format %s (launched %s)" % (key, fname, pt.DeviceScene.NODE_FORMATS[info["format"]])
                check_extend(where, rays, g, o, aimed_at_edges=edge)
            c, _ = dev.trace_rays(rays)
            check_extend("scene %s rebuilt, %s, ptr_trace_rays" % (key, fname), rays, c, o, aimed_at_edges=edge)
            occ, info = dev.connect_rays(any_rays, records_per_slot=2)
            assert np.array_equal(occ, want_any), "scene %s rebuilt, %s: %d rays occluded differently: %s" % (
                key, fname, int((occ != want_any).sum()), _first(any_rays, occ != want_any, ("gpu", occ), ("oracle", want_any)))
            a, _ = dev.trace_rays(any_rays, any_hit=True)
            assert np.array_equal(a["t"] >= 0, want_any), "scene %s rebuilt, %s, any-hit ptr_trace_rays" % (key, fname)
        finally:
            dev.close()


def soup_pose(host, angle, axis, scale, offset):
    t, s = np.eye(4), np.diag([scale[0], scale[1], scale[2], 1.0])
    t[:3, 3] = offset
    return (matrix_of(host, 1).astype(np.float64) @ t @ rotation(axis, angle) @ s).astype(np.float32)


POSE = dict(angle=-1.3, axis=(0.5, -0.4, 1), scale=(-0.9, 1.1, 1.25), offset=(0.15, -0.1, 0.2))


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_soup_hits_are_identical_before_and_after(hosts, fmt):
    host = hosts("soup")
    dev = upload(host, fmt[1])
    try:
        dev.set_mesh_transforms({1: soup_pose(host, **POSE)})
        moved = Moved(host, {1: soup_pose(host, **POSE)})
        rays = ts.mixed_rays(tr.Reference(moved.desc), 20000, 99)
        before, _ = dev.trace_rays(rays)
        assert dev.rebuild_tree(keep_if_better=False)["installed"] == 1
        after, _ = dev.trace_rays(rays)
        assert (before["t"] >= 0).sum() > 500 and before.tobytes() == after.tobytes()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 4. renders
@pytest.mark.parametrize("metal", [0, METAL], ids=["default", "metal"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_soup_renders_are_identical(hosts, fmt, metal):
    host = hosts("soup")
    pose = soup_pose(host, **POSE)
    s = small_settings(host, metal=metal)
    dev, fresh = upload(host, fmt[1]), upload(Moved(host, {1: pose}), fmt[1], dynamic=False)
    try:
        dev.set_mesh_transforms({1: pose})
        before = dev.render_image(s, 4)[0]
        assert dev.rebuild_tree(keep_if_better=False)["installed"] == 1
        after, want = dev.render_image(s, 4)[0], fresh.render_image(s, 4)[0]
        assert want.max() > 0 and np.isfinite(want).all()
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32)), "%d pixels differ across the rebuild" % int((before != after).any(axis=2).sum())
        assert np.array_equal(after.view(np.uint32), want.view(np.uint32)), "%d pixels differ from a fresh upload's" % int((after != want).any(axis=2).sum())
        # an update after the rebuild: another pose against its own fresh upload
        pose2 = soup_pose(host, 2.1, (0.1, 1, 0.3), (1.2, 0.8, 1.0), (0, 0.2, -0.1))
        dev.set_mesh_transforms({1: pose2})
        fresh2 = upload(Moved(host, {1: pose2}), fmt[1], dynamic=False)
        try:
            assert np.array_equal(dev.render_image(s, 4)[0].view(np.uint32), fresh2.render_image(s, 4)[0].view(np.uint32))
        finally:
            fresh2.close()
    finally:
        dev.close()
        fresh.close()


# --------------------------------------------------------------------------------------------------------------------- 5. updates
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("key", ["A", "textured"])
def test_updates_after_a_rebuild_refit_the_new_topology(hosts, key, fmt):
    host = hosts(key)
    dev = upload(host, fmt[1], deformable=True)
    try:
        what = "scene %s, %s" % (key, fmt[0])
        dev.set_mesh_transforms({0: turned(host)})
        assert dev.rebuild_tree(keep_if_better=False)["installed"] == 1
        rebuilt = everything(dev)
        refs = dr.refs_of(rebuilt["boxes"])
        dev.set_mesh_transforms({0: turned(host, angle=-2.0)})
        got, _, _ = check_tree(dev, what + ", moved after the rebuild", collapsed_now=False)
        assert np.array_equal(dr.refs_of(got["boxes"]), refs) and not np.array_equal(got["boxes"], rebuilt["boxes"])
        dev.set_mesh_transforms({0: turned(host)})
        same_arrays(everything(dev), rebuilt, what + ", moved back")
        dev.set_mesh_vertices({0: dsc.displaced(host)})
        got, _, _ = check_tree(dev, what + ", deformed after the rebuild", collapsed_now=False)
        assert np.array_equal(dr.refs_of(got["boxes"]), refs) and not np.array_equal(got["triBounds"], rebuilt["triBounds"])
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 6. handles
def test_a_temporal_sequence_across_a_rebuild(hosts):
    host = hosts("soup")
    outs = []
    for rebuild in (False, True):
        dev = upload(host)
        try:
            temporal = dev.temporal(32, 24)
            seq = []
            for k in range(3):
                s = small_settings(host)
                s.seed = 40 + k
                dev.set_mesh_transforms({1: soup_pose(host, 0.2 * (k + 1), (0.1, 1, 0.3), (1, 1, 1), (0, 0, 0))})
                if rebuild and k == 2:
                    assert dev.rebuild_tree(keep_if_better=False)["installed"] == 1
                out = temporal.step(s, dev.render_image(s, 2)[0])
                seq.append((out["rgb"], out["length"]) + tuple(temporal.records()))
            outs.append(seq)
            temporal.close()
        finally:
            dev.close()
    for k in range(3):
        for a, b in zip(outs[0][k], outs[1][k]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "step %d differs across the rebuild" % k


def test_a_frame_accumulated_across_a_rebuild(hosts):
    host = hosts("soup")
    dev = upload(host)
    try:
        dev.set_mesh_transforms({1: soup_pose(host, **POSE)})
        s = small_settings(host)
        plain, across = dev.frame(s), dev.frame(s)
        plain.accumulate(2)
        plain.accumulate(2)
        across.accumulate(2)
        assert dev.rebuild_tree(keep_if_better=False)["installed"] == 1
        across.accumulate(2)
        a, b = plain.resolve(), across.resolve()
        assert (b[2] == 4).all() and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        plain.close()
        across.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 7. keep if better
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("key", ["A", "D", "strip"])
def test_keep_if_better_installs_only_a_cheaper_tree(hosts, key, fmt):
    host = hosts(key)
    dev = upload(host, fmt[1])
    try:
        for move in (False, True):
            if move:
                dev.set_mesh_transforms({0: turned(host, angle=2.4)})
            before = everything(dev)
            info = dev.rebuild_tree()
            assert info["installed"] == (1 if info["costAfter"] < info["costBefore"] else 0), info
            assert info["costBefore"] == rr.tree_cost(before["boxes"]) or np.isclose(info["costBefore"], rr.tree_cost(before["boxes"]), rtol=1e-9, atol=0)
            if not info["installed"]:
                same_arrays(everything(dev), before, "scene %s, %s: a tree that was not installed" % (key, fmt[0]))
                assert dev.tree_cost() == info["costBefore"]
            else:
                assert dev.tree_cost() == info["costAfter"]
                check_tree(dev, "scene %s, %s: installed" % (key, fmt[0]))
    finally:
        dev.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_scrambled_quads_install_and_get_cheaper(hosts, fmt):
    host = hosts("quads")
    dev = upload(host, fmt[1], deformable=True)
    try:
        fresh = dev.tree_cost()
        dev.set_mesh_vertices({0: rs.scrambled(host)})
        loose = dev.tree_cost()
        info = dev.rebuild_tree()
        assert info["installed"] == 1 and info["costBefore"] == loose and info["costAfter"] < loose and loose > 2.0 * fresh
        assert dev.tree_cost() == info["costAfter"]
        check_tree(dev, "scrambled quads, %s" % fmt[0])
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 8. refusals, no-ops
def test_what_a_rebuild_refuses_and_what_it_leaves_alone(hosts):
    host = hosts("A")
    static = upload(host, dynamic=False)
    try:
        s = small_settings(host)
        before = static.render_image(s, 2)[0]
        with pytest.raises(pt.PtrError, match="not dynamic"):
            static.rebuild_tree()
        with pytest.raises(pt.PtrError, match="not dynamic"):
            static.tree_cost()
        assert np.array_equal(static.render_image(s, 2)[0], before)
    finally:
        static.close()
    dev = upload(host)
    try:
        before = everything(dev)
        err = C.create_string_buffer(256)
        assert pt.load_library().ptr_scene_rebuild_tree(dev._h, 6, None, None, err, len(err)) == 1 and b"flag" in err.value
        same_arrays(everything(dev), before, "after a refused call")
        assert pt.load_library().ptr_scene_rebuild_tree(dev._h, 0, None, None, err, len(err)) == 0   # info may be NULL
        check_tree(dev, "scene A, info NULL")
    finally:
        dev.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_a_single_leaf_is_a_no_op(hosts, fmt):
    host = hosts("F-triangle")
    dev = upload(host, fmt[1])
    try:
        before = everything(dev)
        info = dev.rebuild_tree(keep_if_better=False)
        assert info["installed"] == 0 and info["leaves"] == 1 and info["costBefore"] == info["costAfter"] == 1.0 == dev.tree_cost()
        same_arrays(everything(dev), before, "a scene of one leaf")
    finally:
        dev.close()
