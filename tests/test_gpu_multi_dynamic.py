"""Dynamic scenes on several devices (include/ptr_multi_dynamic.h) on the device: a MultiFrame made with dynamic=True against ONE
single-device dynamic DeviceScene, Frame and Temporal given the same calls.  Every comparison of arrays, images and infos is exact (bit
patterns); tree_cost against float64 numpy is held to test_gpu_rebuild.py's relative 1e-9.  Every test but the refusals runs per node format.

What stands against the numpy references directly, on every partition's scene: the node arrays - dynamic_ref's refit, quantiser and wide
copy through test_gpu_rebuild.py's check_tree - and, after an installed rebuild, the topology, boxes, schedule and level offsets of
rebuild_ref (rebuild_scenes.reference_tree).  dynamic_ref restates no bake: the baked tris / triNormals / triBounds are held against the
single-device scene, which test_gpu_dynamic.py and test_gpu_dynamic_deform.py hold against fresh uploads of the changed description.

64x40 pixels: five 8-row bands, so three partitions own 2 / 2 / 1 of them.  Device lists: one partition, three partitions on device 0,
two partitions of which the second is forced through pinned host memory, and every visible device where there is more than one."""
import ctypes as C

import numpy as np
import pytest
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import deform_device_scenes as dds
import deform_scenes as dsc
import rebuild_ref as rr
import rebuild_scenes as rs
import traversal_scenes as ts
from test_gpu_dynamic_deform import LIGHT, LIGHT_TO, SPHERE_TO, WALL, WALL_TO
from test_gpu_rebuild import FORMATS, FORMAT_IDS, METAL, check_tree, everything, matrix_of, rotation, same_arrays, soup_pose, turned
from test_gpu_traversal import knobs

pt = ts.pt
pytestmark = pytest.mark.gpu

W, H, DEPTH, SPP = 64, 40, 4, 4
LISTS = [[0], [0, 0, 0], [0, -1]] + ([list(range(pt.device_count()))] if pt.device_count() > 1 else [])
LIST_IDS = ["-".join(str(i) for i in ids).replace("--", "-staged") for ids in LISTS]
ALL = dict(deformable=True, primitives=True, vertex_normals=True)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = rs.host_scene(key, tmp_path_factory.mktemp("md_" + key.replace("-", "_")))
        return cache[key]
    return get


def settings_of(host, metal=0, seed=1337):
    s = host.settings_for(width=W, height=H, max_depth=DEPTH, seed=seed)
    s.metalSemantics = metal
    return s


def make(host, ids, env=None, s=None, dynamic=True, **flags):
    """(a MultiFrame on `ids`, the single-device scene it stands against), both uploaded under the same knobs with the same flags."""
    with knobs(env or {}):
        frame = pt.multi_frame(host.desc, s or settings_of(host), device_ids=ids, dynamic=dynamic, **flags)
        dev = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=dynamic, **flags)
    return frame, dev


def arrays_of(scene):
    out = everything(scene)
    del out["rb_pointers"]   # (device addresses: each scene has its own)
    return out


def same_everywhere(frame, ids, dev, what, tree=None):
    """Every partition's arrays are the single-device scene's; tree: check_tree's collapsed_now, to hold them against the references too."""
    want = arrays_of(dev)
    for p in range(len(ids)):
        scene = frame.part_scene(p)
        same_arrays(arrays_of(scene), want, "%s, partition %d of %s" % (what, p, ids))
        if tree is not None:
            check_tree(scene, "%s, partition %d" % (what, p), collapsed_now=tree)
    return want


def on(a, device=0):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:%d" % device)


def tensors(meshes, device=0):
    return {m: tuple(on(a, device) for a in data) for m, data in meshes.items()}


def outputs(frame_like, dev=None, s=None):
    """rgb, cov, count, albedo, normal of a MultiFrame, or of a Frame with its scene's first-hit buffers."""
    if dev is None:
        return frame_like.resolve(want_aovs=True)
    return tuple(frame_like.resolve()) + tuple(dev.render_aovs(s, 0))


def same_outputs(got, want, what):
    for name, a, b in zip(("rgb", "cov", "count", "albedo", "normal"), got, want):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %s differs in %d words" % (
            what, name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def info_of(info):
    return (info.rounds, list(info.activeAfter), info.totalSamples, info.pixelsAtMax)


# --------------------------------------------------------------------------------------------------------------------- 1. arrays
@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("key", ["A", "textured"])
def test_arrays_after_every_update(hosts, key, fmt, ids):
    host = hosts(key)
    frame, dev = make(host, ids, fmt[1], **ALL)
    try:
        what = "scene %s, %s" % (key, fmt[0])
        assert frame.is_dynamic() and frame.dynamic_flags() == dev.dynamic_flags == 7
        same_everywhere(frame, ids, dev, what + ", uploaded")
        steps = [("transforms", lambda t: t.set_mesh_transforms({0: turned(host)}))]
        displaced = dsc.displaced(host)
        assert (len(displaced) == 3) == (key == "textured"), "the textured scene's mesh carries tangents, scene A's does not"
        steps.append(("vertices", lambda t: t.set_mesh_vertices({0: displaced})))
        if host.desc.sphereCount:
            steps.append(("spheres", lambda t: t.set_spheres({0: SPHERE_TO})))
        if host.desc.rectCount > LIGHT:
            steps.append(("rects", lambda t: t.set_rects({LIGHT: LIGHT_TO, WALL: WALL_TO})))
        given = dsc.displaced(host, seed=8, collapse=False)
        steps.append(("device vertices", lambda t: t.set_mesh_vertices_device(tensors({0: given}))))
        computed = (dds.moved(dsc.mesh_data(host)[0], seed=5), None) + tuple(given[2:])
        steps.append(("device vertices, computed normals", lambda t: t.set_mesh_vertices_device(tensors({0: computed}))))
        for name, step in steps:
            want, got = step(dev), step(frame)
            same_everywhere(frame, ids, dev, what + ", " + name, tree=False)
            assert got["parts"] == len(ids) and len(got["partSeconds"]) == len(ids) and min(got["partSeconds"]) > 0
            assert 0 < got["distributeSeconds"] <= got["totalSeconds"] and max(got["partSeconds"]) <= got["totalSeconds"]
            assert got["stagedParts"] == (sum(1 for i in ids if i < 0) if name.startswith("device") else 0), (name, got)
            for field in ("trianglesMoved", "nodes", "levels", "wideNodes", "sceneLo", "sceneHi", "gridOrigin", "gridCell", "cellOverExtent"):
                assert got[field] == want[field], (name, field)
    finally:
        frame.close()
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 2. frames
@pytest.mark.parametrize("metal", [0, METAL], ids=["default", "metal"])
@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_frames_over_three_poses_and_a_refine(hosts, fmt, ids, metal):
    host = hosts("soup")
    s = settings_of(host, metal)
    frame, dev = make(host, ids, fmt[1], s=s)
    single = dev.frame(s)
    try:
        for k in range(3):
            pose = {1: soup_pose(host, 0.4 * (k + 1), (0.1, 1, 0.3), (1, 1 + 0.1 * k, 1), (0, 0.1 * k, 0))}
            dev.set_mesh_transforms(pose)
            frame.set_mesh_transforms(pose)
            single.reset()
            frame.reset()
            single.accumulate(SPP)
            frame.accumulate(SPP)
            want = outputs(single, dev, s)
            assert (want[2] == SPP).all() and want[0].max() > 0 and (want[3][..., 3] > 0).any()
            same_outputs(outputs(frame), want, "pose %d on %s" % (k, ids))
        e = single.export_state()["e"]
        params = pt.PtrAdaptiveParams(SPP, 12, 4, float(np.median(e[e > 0])))
        _, want_info = single.refine(params)
        _, got_info = frame.refine(params)
        assert 0 < want_info.activeAfter[0] < W * H, "the threshold leaves some pixels active and settles others"
        assert info_of(got_info) == info_of(want_info)
        same_outputs(outputs(frame), outputs(single, dev, s), "after the refine on %s" % ids)
    finally:
        single.close()
        frame.close()
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 3. no reset
@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_accumulating_across_an_update_without_a_reset(hosts, fmt, ids):
    host = hosts("soup")
    s = settings_of(host)
    frame, dev = make(host, ids, fmt[1], s=s)
    single = dev.frame(s)
    try:
        pose = {1: soup_pose(host, 0.9, (0.1, 1, 0.3), (1, 1, 1), (0, 0.3, 0))}
        for t in (single, frame):
            t.accumulate(2)
        before = frame.export_state()
        dev.set_mesh_transforms(pose)
        frame.set_mesh_transforms(pose)
        after = frame.export_state()
        for name in before:
            assert np.array_equal(before[name].view(np.uint32), after[name].view(np.uint32)), "an update touched the sample state: " + name
        for t in (single, frame):
            t.accumulate(2)
        want = outputs(single, dev, s)
        assert (want[2] == 4).all()
        same_outputs(outputs(frame), want, "a blur over two poses on %s" % ids)
    finally:
        single.close()
        frame.close()
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 4. device data
@pytest.mark.parametrize("ids", [[0, 0, 0], [0, -1]], ids=["0-0-0", "0-staged1"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_device_data_on_a_torch_stream_and_a_refused_nan(hosts, fmt, ids):
    host = hosts("A")
    s = settings_of(host)
    frame, dev = make(host, ids, fmt[1], s=s, **ALL)
    try:
        base = dsc.mesh_data(host)[0]
        step = (dds.moved(base, seed=77) - base).astype(np.float32)
        d_base, d_step = on(base), on(step)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d_pos = d_base + d_step          # enqueued on `stream`; the call reads it there (stream=None: torch's current stream)
            info = frame.set_mesh_vertices_device({0: (d_pos, None)})
        dev.set_mesh_vertices_device({0: (on(base + step), None)})
        assert info["stagedParts"] == sum(1 for i in ids if i < 0) and info["parts"] == len(ids)
        want = same_everywhere(frame, ids, dev, "positions made on a torch stream")
        frame.accumulate(SPP)
        image = outputs(frame)
        # a NaN in one component: refused on the device, nothing changed anywhere
        bad = base.copy()
        bad[len(bad) // 2, 1] = np.nan
        for normals in (None, dsc.mesh_data(host)[1]):
            with pytest.raises(pt.PtrError, match="ptr_multi_frame_set_mesh_vertices_device: mesh 0 has a non-finite position component"):
                frame.set_mesh_vertices_device({0: (on(bad), on(normals))})
        for p in range(len(ids)):
            same_arrays(arrays_of(frame.part_scene(p)), want, "after the refused call, partition %d" % p)
        same_outputs(outputs(frame), image, "the resolve after the refused call")
        # ... and the frame goes on: the next call is the single-device scene's again
        pose = tensors({0: dsc.displaced(host, seed=4, collapse=False)})
        dev.set_mesh_vertices_device(pose)
        frame.set_mesh_vertices_device(pose)
        same_everywhere(frame, ids, dev, "the call after the refused one")
    finally:
        frame.close()
        dev.close()


@pytest.mark.skipif(pt.device_count() < 2, reason="needs two devices")
def test_device_data_on_the_second_device(hosts):
    host = hosts("A")
    frame, dev = make(host, [0, 1], **ALL)
    try:
        for device in (1, 0):
            data = {0: dsc.displaced(host, seed=10 + device, collapse=False)}
            dev.set_mesh_vertices_device(tensors(data, 0))
            info = frame.set_mesh_vertices_device(tensors(data, device))
            same_everywhere(frame, [0, 1], dev, "arrays on device %d" % device)
            print("arrays on device %d: %s" % (device, {k: info[k] for k in ("stagedParts", "totalSeconds", "distributeSeconds", "partSeconds")}))
    finally:
        frame.close()
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 5. rebuild
@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_rebuild_agreement(hosts, fmt, ids):
    host = hosts("quads")
    frame, dev = make(host, ids, fmt[1], deformable=True)
    counts = ("installed", "costBefore", "costAfter", "nodes", "levels", "wideNodes", "wideDepth", "leaves")
    try:
        what = "quads, %s on %s" % (fmt[0], ids)

        def both(keep):
            last = frame.part_scene(len(ids) - 1)
            before = last.arrays(["boxes", "triBounds", "sphereBounds"])
            nodes, schedule, offsets = rs.reference_tree(before["boxes"], before["triBounds"], before["sphereBounds"])   # rebuild_ref, directly
            want, got = dev.rebuild_tree(keep_if_better=keep), frame.rebuild_tree(keep_if_better=keep)
            if want["installed"]:
                after, rb = last.arrays(["boxes"]), last.rebuild_arrays(["schedule", "levelOffsets"])
                same_arrays(after, {"boxes": nodes}, what + ": the last partition's tree against rebuild_ref")
                assert np.array_equal(rb["schedule"], schedule) and np.array_equal(rb["levelOffsets"], offsets), what
            print("%s, keep_if_better=%s: %s" % (what, keep, {k: want[k] for k in counts}))
            assert [got[k] for k in counts] == [want[k] for k in counts], (what, got, want)
            arrays = same_everywhere(frame, ids, dev, what, tree=bool(want["installed"]))
            cost = frame.tree_cost()
            assert cost == dev.tree_cost() == (want["costAfter"] if want["installed"] else want["costBefore"])
            assert np.isclose(cost, rr.tree_cost(arrays["boxes"]), rtol=1e-9, atol=0), what
            return want

        # a 5 degree turn of the fresh upload that does not install: the radix tree is no better than the lightly refitted SAH tree
        turn = {0: (matrix_of(host).astype(np.float64) @ rotation((0.3, 1.0, -0.45), np.radians(5.0))).astype(np.float32)}
        dev.set_mesh_transforms(turn)
        frame.set_mesh_transforms(turn)
        info = both(True)
        assert info["installed"] == 0 and not info["costAfter"] < info["costBefore"]
        # a twist that installs: every quad moved to the place of another
        twist = {0: rs.scrambled(host)}
        dev.set_mesh_vertices(twist)
        frame.set_mesh_vertices(twist)
        info = both(True)
        assert info["installed"] == 1 and info["costAfter"] < info["costBefore"]
        # updates after the install refit the new topology on every partition
        dev.set_mesh_transforms({0: matrix_of(host)})
        frame.set_mesh_transforms({0: matrix_of(host)})
        same_everywhere(frame, ids, dev, what + ", an update on the new topology", tree=False)
        # without the flag it is installed whatever it costs
        assert both(False)["installed"] == 1
        dev.set_mesh_vertices({0: dsc.original(host)})
        frame.set_mesh_vertices({0: dsc.original(host)})
        same_everywhere(frame, ids, dev, what + ", deformed back after two rebuilds", tree=False)
    finally:
        frame.close()
        dev.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_a_frame_rendered_after_an_install_equals_the_frame_before_it(hosts, fmt):
    host = hosts("soup")
    s = settings_of(host)
    frame, dev = make(host, [0, 0, 0], fmt[1], s=s)
    try:
        pose = {1: soup_pose(host, -1.3, (0.5, -0.4, 1), (-0.9, 1.1, 1.25), (0.15, -0.1, 0.2))}
        frame.set_mesh_transforms(pose)
        frame.accumulate(SPP)
        before = outputs(frame)
        assert frame.rebuild_tree(keep_if_better=False)["installed"] == 1
        frame.reset()
        frame.accumulate(SPP)
        same_outputs(outputs(frame), before, "the tie-free soup across an install")
    finally:
        frame.close()
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 6. pipeline
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_turntable_pipeline_on_the_first_device(hosts, fmt):
    """update -> reset -> accumulate -> resolve_device -> temporal(cov).step_device on partition 0's scene -> the covariance denoiser, with
    no host round trip, on three partitions and on a single-device scene, Frame and Temporal."""
    host = hosts("soup")
    frame, dev = make(host, [0, 0, 0], fmt[1])
    single = dev.frame(settings_of(host))
    handles = {"multi": frame.temporal(W, H, cov=True), "single": dev.temporal(W, H, cov=True)}
    n = W * H
    zeros = lambda c: torch.zeros(n * c, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream(0).cuda_stream
    try:
        for k in range(4):
            s = settings_of(host, seed=40 + k)
            pose = {1: soup_pose(host, 0.2 * (k + 1), (0.1, 1, 0.3), (1, 1, 1), (0, 0, 0))}
            results = {}
            for name, target, accumulator in (("multi", frame, frame), ("single", dev, single)):
                target.set_mesh_transforms(pose)
                accumulator.reset(s)
                accumulator.accumulate(SPP)
                d_rgb, d_cov, d_count = zeros(3), zeros(6), torch.zeros(n, dtype=torch.int32, device="cuda:0")
                accumulator.resolve_device(d_rgb.data_ptr(), d_cov.data_ptr(), d_count.data_ptr(), stream)
                outs = {o: zeros(c) for o, c in (("rgb", 3), ("cov", 6), ("length", 1), ("albedo", 4), ("normal", 4))}
                handles[name].step_device(s, d_rgb, outs["rgb"], outs["length"], outs["albedo"], outs["normal"], cov=d_cov, out_cov=outs["cov"])
                torch.cuda.synchronize()
                temporal = {o: t.cpu().numpy().copy() for o, t in outs.items()}
                pt.denoise_device(outs["rgb"].data_ptr(), outs["albedo"].data_ptr(), outs["normal"].data_ptr(), W, H, stream=stream,
                                  d_cov=outs["cov"].data_ptr())
                torch.cuda.synchronize()
                results[name] = dict(temporal, resolved=d_rgb.cpu().numpy(), resolved_cov=d_cov.cpu().numpy(), count=d_count.cpu().numpy(),
                                     denoised=outs["rgb"].cpu().numpy())
            assert results["single"]["resolved"].max() > 0 and (results["single"]["count"] == SPP).all()
            for o, want in results["single"].items():
                got = results["multi"][o]
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "frame %d: %s differs in %d words" % (
                    k, o, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    finally:
        for t in handles.values():
            t.close()
        single.close()
        frame.close()
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 7. checkpoints
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_a_checkpoint_does_not_carry_the_pose_and_passes_between_device_counts(hosts, fmt):
    host = hosts("soup")
    s = settings_of(host)
    pose_b = {1: soup_pose(host, 1.1, (0.1, 1, 0.3), (1, 0.9, 1), (0, 0.2, 0.1))}
    three, dev = make(host, [0, 0, 0], fmt[1], s=s)
    one, dev_one = make(host, [0], fmt[1], s=s)
    whole, into = dev.frame(s), dev_one.frame(s)
    try:
        for t in (three, dev, one, dev_one):
            t.set_mesh_transforms(pose_b)
        whole.accumulate(SPP)
        whole.accumulate(SPP)
        three.accumulate(SPP)
        saved = three.export_state()
        one.import_state(saved)
        into.import_state(saved)
        for t in (three, one, into):
            t.accumulate(SPP)
        want = outputs(whole, dev, s)
        assert (want[2] == 2 * SPP).all()
        same_outputs(outputs(three), want, "three partitions, never interrupted")
        same_outputs(outputs(one), want, "continued on one partition")
        same_outputs(outputs(into, dev_one, s), want, "continued in a single-device Frame")
    finally:
        for t in (whole, into, three, one, dev, dev_one):
            t.close()


# --------------------------------------------------------------------------------------------------------------------- 8. refusals
def test_a_static_frame_refuses_every_call_and_stays_usable(hosts):
    host = hosts("A")
    s = settings_of(host)
    with knobs({}):
        frame = pt.multi_frame(host.desc, s, device_ids=[0, 0, 0])
    try:
        assert not frame.is_dynamic() and frame.dynamic_flags() == 0
        frame.accumulate(SPP)
        before = outputs(frame)
        data = dsc.displaced(host)
        calls = [("set_mesh_transforms", lambda: frame.set_mesh_transforms({0: turned(host)}), "the scene is not dynamic"),
                 ("set_mesh_vertices", lambda: frame.set_mesh_vertices({0: data}), "the scene is not deformable"),
                 ("set_mesh_vertices_device", lambda: frame.set_mesh_vertices_device(tensors({0: data})), "the scene is not deformable"),
                 ("set_spheres", lambda: frame.set_spheres({0: SPHERE_TO}), "the scene does not keep its primitives"),
                 ("set_rects", lambda: frame.set_rects({LIGHT: LIGHT_TO}), "the scene does not keep its primitives"),
                 ("tree_cost", frame.tree_cost, "the scene is not dynamic"), ("rebuild_tree", frame.rebuild_tree, "the scene is not dynamic")]
        for name, call, words in calls:
            with pytest.raises(pt.PtrError, match="^ptr_multi_frame_%s: %s" % (name, words)):
                call()
        same_outputs(outputs(frame), before, "a static frame after the refused calls")
        frame.reset()
        frame.accumulate(SPP)
        same_outputs(outputs(frame), before, "a static frame goes on rendering")
    finally:
        frame.close()


def test_what_a_dynamic_frame_refuses(hosts):
    host = hosts("A")
    s = settings_of(host)
    plain, dev = make(host, [0, 0, 0], s=s)   # flags 0: ptr_scene_upload_dynamic
    full, dev_full = make(host, [0, -1], s=s, **ALL)
    lib = pt.load_library()
    try:
        data = dsc.displaced(host)
        # the single-device words behind the frame's function name
        for target, name in ((dev, "ptr_scene_"), (plain, "ptr_multi_frame_")):
            with pytest.raises(pt.PtrError, match="^%sset_mesh_vertices: the scene is not deformable \\(upload it with ptr_scene_upload_dynamic_ex" % name):
                target.set_mesh_vertices({0: data})
            with pytest.raises(pt.PtrError, match="^%sset_mesh_vertices_device: the scene is not deformable" % name):
                target.set_mesh_vertices_device(tensors({0: data}))
            with pytest.raises(pt.PtrError, match="^%sset_spheres: the scene does not keep its primitives" % name):
                target.set_spheres({0: SPHERE_TO})
        full.accumulate(SPP)
        image, arrays = outputs(full), [arrays_of(full.part_scene(p)) for p in range(2)]
        meshes = host.desc.meshCount
        singular = np.diag([1.0, 0.0, 1.0, 1.0]).astype(np.float32)
        nan = np.eye(4, dtype=np.float32)
        nan[1, 2] = np.nan
        for target, name in ((dev_full, "ptr_scene_"), (full, "ptr_multi_frame_")):
            for call, words in ((lambda: target.set_mesh_transforms({meshes: np.eye(4)}), "set_mesh_transforms: mesh index %d out of range" % meshes),
                                (lambda: target.set_mesh_transforms({0: singular}), "set_mesh_transforms: the matrix of mesh 0 has a zero 3x3 determinant"),
                                (lambda: target.set_mesh_transforms({0: nan}), "set_mesh_transforms: the matrix of mesh 0 has a non-finite entry"),
                                (lambda: target.set_mesh_vertices({0: (data[0][:-1], data[1][:-1])}), "set_mesh_vertices: mesh 0 was uploaded with"),
                                (lambda: target.set_spheres({host.desc.sphereCount: SPHERE_TO}), "set_spheres: sphere index %d out of range" % host.desc.sphereCount),
                                (lambda: target.set_rects({LIGHT: dict(LIGHT_TO, edgeV=(0.0, 0.0, 1.0))}), "set_rects: rectangle %d has cross" % LIGHT)):
                with pytest.raises(pt.PtrError, match="^" + name + words):
                    call()
        # an index named twice, src_device past the visible ones: through the C interface
        err = C.create_string_buffer(256)
        twice = (pt.PtrMeshTransform * 2)()
        for item in twice:
            item.meshIndex = 0
            item.localToWorld[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
        assert lib.ptr_multi_frame_set_mesh_transforms(full._h, twice, 2, None, err, len(err)) == 1
        assert err.value == b"ptr_multi_frame_set_mesh_transforms: mesh index 0 named twice"
        items, _ = pt._vertex_device_items(tensors({0: data}), 0)
        assert lib.ptr_multi_frame_set_mesh_vertices_device(full._h, items, 1, pt.device_count(), None, None, err, len(err)) == 1
        assert err.value == b"ptr_multi_frame_set_mesh_vertices_device: no such HIP device"
        # a partition's scene is updated through the frame alone
        with pytest.raises(pt.PtrError, match="through its MultiFrame"):
            full.part_scene(1).set_mesh_transforms({0: turned(host)})
        for p in range(2):
            same_arrays(arrays_of(full.part_scene(p)), arrays[p], "after the refused calls, partition %d" % p)
        same_outputs(outputs(full), image, "the resolve after the refused calls")
    finally:
        for t in (plain, full, dev, dev_full):
            t.close()
