"""include/ptr_deform_device.h on the device: ptr_scene_set_mesh_vertices_device against ptr_scene_set_mesh_vertices with the same data,
and the normals k_dyn_vertex_normals computes against the numpy restatement (tests/deform_device_ref.py) and against a fresh upload that
carries the reference's normals.  Every comparison of arrays and images is exact (bit patterns)."""
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import deform_device_ref as ref
import deform_device_scenes as dds
import deform_scenes as dsc
import traversal_scenes as ts
from test_gpu_dynamic import FORMATS, FORMAT_IDS, matrix_of, same_arrays, small_settings, soup_scene, t1_t2
from test_gpu_dynamic_deform import assert_same_image, same_by_meta, tree_follows_the_bounds, waved
from test_gpu_traversal import knobs

pt = ts.pt
pytestmark = pytest.mark.gpu

GOLDEN = ts.GOLDEN
METAL = pt.PTR_METAL_FACE_NORMAL | pt.PTR_METAL_SPECULAR | pt.PTR_METAL_CLAMPS


def upload(holder, env=None, vertex_normals=True, dynamic=True):
    with knobs(env or {}):
        return pt.DeviceScene(holder.desc, 0, keepalive=holder, dynamic=dynamic, deformable=dynamic, primitives=dynamic, vertex_normals=dynamic and vertex_normals)


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def tensors(meshes):
    """{mesh: (positions, normals or None[, tangents])} of numpy arrays as torch tensors on the device."""
    return {m: tuple(None if a is None else on_device(a) for a in data) for m, data in meshes.items()}


def three_mesh_scene(tmp):
    """Two meshes with triangles (a pair, a strip that crosses a block) and a third one that is given none."""
    ts._write_obj(tmp / "pair.obj", [(-1, -0.5, 0.2), (1, -0.4, -0.1), (0.1, 1, 0), (1.2, 1.1, 0.3)], [(0, 1, 2), (2, 1, 3)])
    verts, faces = dds.strip(259)
    ts._write_obj(tmp / "strip.obj", verts, faces)
    ts._write_obj(tmp / "one.obj", [(-1, -0.5, 0.2), (1, -0.4, -0.1), (0.1, 1, 0)], [(0, 1, 2)])
    p = tmp / "three.scene"
    p.write_text(ts.HEAD + "mesh path=pair.obj material=0\nmesh path=strip.obj translate=0,0,1 material=0\nmesh path=one.obj translate=0,2,0 material=0\n")
    bare = dsc.Changed(ts.load(p, str(tmp)))
    bare._meshes[2].indexCount = 0
    return bare


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    cache = {}

    def get(key):
        if key not in cache:
            tmp = tmp_path_factory.mktemp("deform_device_" + key.replace("-", "_"))
            if key == "textured":
                cache[key] = pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN)
            elif key == "A":
                cache[key] = ts.scene_a()
            elif key == "soup":
                cache[key] = soup_scene(tmp)
            elif key == "three":
                cache[key] = three_mesh_scene(tmp)
            elif key in dds.MESHES:
                cache[key] = dds.remeshed(tmp, key)
            else:
                cache[key] = ts.scene_f(tmp, key[2:])
        return cache[key]
    return get


def meshes_of(host):
    return [m for m in range(host.desc.meshCount) if host.desc.meshes[m].indexCount >= 3]


def deformations(host, seed=3, collapse=True):
    return {m: dsc.displaced(host, m, seed + m, collapse) for m in meshes_of(host)}


def without_normals(meshes):
    return {m: (data[0], None) + tuple(data[2:]) for m, data in meshes.items()}


def with_reference_normals(host, meshes):
    """The same vertex data with tests/deform_device_ref.py's normals of the new positions in place of the given ones."""
    out = {}
    for m, data in meshes.items():
        out[m] = (data[0], ref.normals(data[0], dsc.mesh_data(host, m)[3])) + tuple(data[2:])
        assert np.isfinite(out[m][1]).all()
    return out


# --------------------------------------------------------------------------------------------------------------------- 1. given normals
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("key", ["A", "textured", "F-triangle", "fan"])
def test_given_normals_equal_the_host_pointer_call(hosts, key, fmt):
    host = hosts(key)
    new = deformations(host)
    dev, twin = upload(host, fmt[1]), upload(host, fmt[1], vertex_normals=False)
    try:
        assert dev.dynamic_flags == 7 and twin.dynamic_flags == 3
        first = dev.arrays()
        same_arrays(twin.arrays(), first, "scene %s, %s: the uploads with and without the flag" % (key, fmt[0]))
        a, b = dev.set_mesh_vertices_device(tensors(new)), twin.set_mesh_vertices(new)
        got = dev.arrays()
        same_arrays(got, twin.arrays(), "scene %s, %s: device pointers against host pointers" % (key, fmt[0]))
        assert not np.array_equal(got["tris"], first["tris"]) and not np.array_equal(got["objNrm"], first["objNrm"])
        if key == "textured":
            assert len(got["objTan"]) and not np.array_equal(got["objTan"], first["objTan"])
        for name in ("trianglesMoved", "nodes", "levels", "wideNodes", "sceneLo", "sceneHi", "gridOrigin", "gridCell", "cellOverExtent"):
            assert a[name] == b[name], name
        assert a["trianglesMoved"] == sum(host.desc.meshes[m].indexCount // 3 for m in range(host.desc.meshCount))
        # and a scene without the flag takes device pointers all the same, as long as the normals come with them
        twin.set_mesh_vertices_device(tensors(deformations(host, seed=40)))
        dev.set_mesh_vertices(deformations(host, seed=40))
        same_arrays(twin.arrays(), dev.arrays(), "scene %s, %s: the calls swapped" % (key, fmt[0]))
    finally:
        dev.close()
        twin.close()


# --------------------------------------------------------------------------------------------------------------------- 2. several meshes
def test_several_meshes_in_one_call_one_of_them_without_triangles(hosts):
    host = hosts("three")
    assert host.desc.meshCount == 3 and meshes_of(host) == [0, 1]
    new = deformations(host, seed=17)
    spare = (np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32))   # for the mesh without triangles: accepted, changes nothing
    dev, twin = upload(host), upload(host, vertex_normals=False)
    try:
        a = dev.set_mesh_vertices_device(tensors({2: spare, 1: new[1], 0: new[0]}))
        b = twin.set_mesh_vertices({2: spare, 1: new[1], 0: new[0]})
        assert a["trianglesMoved"] == b["trianglesMoved"] == 2 + 257
        same_arrays(dev.arrays(), twin.arrays(), "three meshes in one call")
        # and with the normals of both computed in that one call
        info = dev.set_mesh_vertices_device(tensors(without_normals({2: spare, 0: new[0], 1: new[1]})))
        fresh = upload(dsc.Changed(host, vertices=with_reference_normals(host, new)))
        try:
            got = dev.arrays()
            same_by_meta(got, fresh.arrays(), "three meshes, computed normals")
            tree_follows_the_bounds(host, got, info, "three meshes, computed normals")
        finally:
            fresh.close()
    finally:
        dev.close()
        twin.close()


# --------------------------------------------------------------------------------------------------------------------- 3. pointer layouts
def corner_normals(host, got, mesh, normals):
    """objNrm of `mesh` in downloaded arrays against per-vertex normals gathered through the corner table: rows and what they should be."""
    t = pt.debug_dynamic_tables(host.desc, ["meshTris", "meshCorners", "meshTriOffsets"])
    rows = slice(t["meshTriOffsets"][mesh], t["meshTriOffsets"][mesh + 1])
    have = got["objNrm"][t["meshTris"][rows]]
    want = np.zeros_like(have)
    want[..., :3] = normals[t["meshCorners"][rows]]
    return have, want


@pytest.mark.parametrize("vertices", [1, 255, 256, 257])
def test_block_edges_and_a_view_that_is_only_4_byte_aligned(hosts, vertices):
    host = hosts("strip%d" % vertices)
    assert host.desc.meshes[0].vertexCount == vertices
    pos = dds.moved(host.positions, seed=vertices)
    nrm = np.random.default_rng(vertices).normal(size=pos.shape).astype(np.float32)
    dev, twin = upload(host), upload(host, vertex_normals=False)
    try:
        # each array 4 B into an allocation of its own: 16 B alignment is gone, 4 B is what the call asks for
        views = []
        for a in (pos, nrm):
            big = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
            view = big[1:1 + a.size].view(-1, 3)
            view.copy_(torch.from_numpy(a))
            assert view.is_contiguous() and view.data_ptr() % 16 == 4
            views.append(view)
        dev.set_mesh_vertices_device({0: tuple(views)})
        twin.set_mesh_vertices({0: (pos, nrm)})
        same_arrays(dev.arrays(), twin.arrays(), "a strip of %d vertices from views 4 B into their allocations" % vertices)
        dev.set_mesh_vertices_device({0: (views[0], None)})
        have, want = corner_normals(host, dev.arrays(), 0, ref.normals(pos, host.indices))
        assert np.array_equal(have.view(np.uint32), want.view(np.uint32)), vertices
        assert vertices == 1 or np.abs(want).max() > 0.5
    finally:
        dev.close()
        twin.close()


# --------------------------------------------------------------------------------------------------------------------- 4. computed normals
@pytest.mark.parametrize("key", ["A", "textured", "F-triangle", "F-coincident", "fan", "cancel", "odd"])
def test_computed_normals_equal_the_reference_and_a_fresh_upload(hosts, key):
    host = hosts(key)
    new = deformations(host, seed=9, collapse=key != "cancel")   # (a collapsed first triangle would cancel by being a point)
    want = with_reference_normals(host, new)
    dev, fresh = upload(host), upload(dsc.Changed(host, vertices=want))
    try:
        info = dev.set_mesh_vertices_device(tensors(without_normals(new)))
        got = dev.arrays()
        what = "scene %s, normals computed on the device" % key
        for m in meshes_of(host):
            have, rows = corner_normals(host, got, m, want[m][1])
            diff = (have.view(np.uint32) != rows.view(np.uint32)).any(axis=2)
            assert not diff.any(), "%s: mesh %d, %d corners differ, first %s" % (what, m, int(diff.sum()), [
                (int(e), int(c), have[e, c].tolist(), rows[e, c].tolist()) for e, c in list(zip(*np.nonzero(diff)))[:3]])
        same_by_meta(got, fresh.arrays(), what)
        tree_follows_the_bounds(host, got, info, what)
        if key == "fan":
            assert (dsc.mesh_data(host)[3] == 0).any(axis=1).sum() == 70, "the hub's sum runs over more entries than a wave has lanes"
        if key == "cancel":
            p0, p1, p2 = new[0][0][:3]
            assert np.abs(np.cross(p1 - p0, p2 - p0)).min() > 1e-3, "neither winding's cross product is zero"
            assert np.array_equal(want[0][1][0].view(np.uint32), np.zeros(3, np.uint32)), "at vertex 0 the two windings cancel to +0"
            assert (np.linalg.norm(want[0][1][1:], axis=1) > 0.99).all()
        if key == "odd":
            assert np.array_equal(want[0][1][5], np.zeros(3, np.float32)), "the unreferenced vertex"
    finally:
        dev.close()
        fresh.close()


# --------------------------------------------------------------------------------------------------------------------- 5. stacked updates
def test_a_rigid_move_then_a_device_deformation_and_back(hosts):
    host = hosts("textured")
    last = host.desc.meshCount - 1
    m = t1_t2(host, last)[1]
    new = deformations(host, seed=21)
    want = with_reference_normals(host, new)
    dev, fresh = upload(host), upload(dsc.Changed(host, vertices=want, matrices={last: m}))
    try:
        first = dev.arrays()
        dev.set_mesh_transforms({last: m})
        info = dev.set_mesh_vertices_device(tensors(without_normals(new)))   # bakes under the matrix the mesh has now
        got = dev.arrays()
        same_by_meta(got, fresh.arrays(), "the textured scene moved, then deformed from device data")
        tree_follows_the_bounds(host, got, info, "the textured scene moved, then deformed from device data")
        dev.set_mesh_vertices_device(tensors({k: dsc.original(host, k) for k in meshes_of(host)}))
        dev.set_mesh_transforms({last: matrix_of(host, last)})
        same_arrays(dev.arrays(), first, "the textured scene after restoring vertices and matrix")
    finally:
        dev.close()
        fresh.close()


# --------------------------------------------------------------------------------------------------------------------- 6. a render
@pytest.mark.parametrize("metal", [0, METAL], ids=["default", "metal"])
def test_render_with_computed_normals_equals_a_fresh_uploads(hosts, metal):
    host = hosts("soup")
    states = [{m: waved(host, m, phase) for m in range(2)} for phase in (0.4, 2.9)]
    s = small_settings(host, 64, 48, 4, metal)
    dev, fresh = upload(host), upload(dsc.Changed(host, vertices=with_reference_normals(host, states[1])), dynamic=False)
    try:
        before = dev.render_image(s, 4)[0]
        for state in states:
            dev.set_mesh_vertices_device(tensors(without_normals(state)))
        got = dev.render_image(s, 4)[0]
        assert_same_image(got, fresh.render_image(s, 4)[0], "the soup deformed from device positions, normals computed")
        assert not np.array_equal(got, before)
    finally:
        dev.close()
        fresh.close()


# --------------------------------------------------------------------------------------------------------------------- 7. refusals
def raw_call(dev, items, count=None, pointer=True, stream=None):
    """ptr_scene_set_mesh_vertices_device with addresses as given: [(mesh, vertexCount, positions, normals, tangents)], 0 for null."""
    arr = (pt.PtrMeshVerticesDevice * max(len(items), 1))()
    for k, (index, vc, p, q, t) in enumerate(items):
        arr[k].meshIndex, arr[k].vertexCount = index, vc
        arr[k].positions, arr[k].normals, arr[k].tangents = p or None, q or None, t or None
    err = C.create_string_buffer(512)
    rc = pt.load_library().ptr_scene_set_mesh_vertices_device(dev._h, arr if pointer else None, len(items) if count is None else count, C.c_void_p(stream), None, err, len(err))
    torch.cuda.synchronize()
    return rc, err.value.decode()


def test_what_the_device_pointer_call_refuses(hosts):
    host = hosts("textured")
    dev = upload(host)
    try:
        before = dev.arrays()
        pos, nrm, tan = dsc.original(host, 0)
        n = len(pos)
        idx = dsc.mesh_data(host, 0)[3]

        held = []   # every tensor whose address a call is given stays allocated until the end of the test

        def address(t):
            held.append(t)
            return t.data_ptr()

        def poisoned(a, value):
            b = a.copy()
            b[n // 2, 1] = value
            return address(on_device(b))

        huge = pos.copy()
        huge[idx[0]] = np.array([(3e38, 0, 0), (-3e38, 0, 0), (0, 3e38, 0)], np.float32)
        assert np.isfinite(huge).all() and not np.isfinite(ref.normals(huge, idx)).all()
        d_pos, d_nrm, d_tan, d_huge = on_device(pos), on_device(nrm), on_device(tan), on_device(huge)
        p, q, t = d_pos.data_ptr(), d_nrm.data_ptr(), d_tan.data_ptr()
        host_pos = np.ascontiguousarray(pos)
        second = [address(on_device(a)) for a in dsc.original(host, 1)]
        second = (1, host.desc.meshes[1].vertexCount) + tuple(second) + (0,) * (3 - len(second))
        cases = [("NaN position", raw_call(dev, [(0, n, poisoned(pos, np.nan), q, t)]), "mesh 0 has a non-finite position component"),
                 ("infinite normal", raw_call(dev, [(0, n, p, poisoned(nrm, np.inf), t)]), "mesh 0 has a non-finite normal component"),
                 ("NaN tangent", raw_call(dev, [(0, n, p, q, poisoned(tan, np.nan))]), "mesh 0 has a non-finite tangent component"),
                 ("position ahead of tangent", raw_call(dev, [(0, n, poisoned(pos, np.inf), q, poisoned(tan, np.nan))]), "non-finite position"),
                 ("second mesh fine, first not", raw_call(dev, [second, (0, n, p, poisoned(nrm, np.nan), t)]), "mesh 0 has a non-finite normal"),
                 ("computed normal overflows", raw_call(dev, [(0, n, d_huge.data_ptr(), 0, t)]), "mesh 0 has a non-finite normal component"),
                 ("host pointer", raw_call(dev, [(0, n, host_pos.ctypes.data, q, t)]), "position array of mesh 0 is host memory"),
                 ("host normals", raw_call(dev, [(0, n, p, nrm.ctypes.data, t)]), "normal array of mesh 0 is host memory"),
                 ("pinned host pointer", raw_call(dev, [(0, n, p, q, address(torch.from_numpy(tan).pin_memory()))]), "tangent array of mesh 0 is .*host memory"),
                 ("not 4 B aligned", raw_call(dev, [(0, n, p + 2, q, t)]), "position array of mesh 0 is not 4 B aligned"),
                 ("tangents missing", raw_call(dev, [(0, n, p, q, 0)]), "with tangents and is given none"),
                 ("vertex count", raw_call(dev, [(0, n - 1, p, q, t)]), "was uploaded with %d vertices, not vertexCount %d" % (n, n - 1)),
                 ("null positions", raw_call(dev, [(0, n, 0, q, t)]), "null positions"),
                 ("null list", raw_call(dev, [], 1, False), "null mesh list"), ("count 0", raw_call(dev, [(0, n, p, q, t)], 0), "count is 0"),
                 ("index out of range", raw_call(dev, [(host.desc.meshCount, n, p, q, t)]), "out of range"),
                 ("index named twice", raw_call(dev, [(0, n, p, q, t), (0, n, p, q, t)]), "named twice")]
        for name, (rc, message), pattern in cases:
            assert rc != 0 and message.startswith("ptr_scene_set_mesh_vertices_device:") and re.search(pattern, message), (name, rc, message)
        same_arrays(dev.arrays(), before, "after the refused ptr_scene_set_mesh_vertices_device calls")
        # the wrapper refuses what is no float32 [n, 3] / [n, 4] tensor on the scene's device before it calls the library
        wrong = [("dtype", (d_pos.double(), d_nrm, d_tan), "float32"), ("shape", (d_tan, d_nrm, d_tan), r"shape \(%d, 4\)" % n),
                 ("shape", (d_pos, d_nrm[:-1], d_tan), "shape"), ("shape", (d_pos.reshape(-1), d_nrm, d_tan), "shape"),
                 ("device", (torch.from_numpy(pos), d_nrm, d_tan), "are on cpu"), ("layout", (d_pos, d_nrm, d_tan.t().contiguous().t()), "not contiguous"),
                 ("type", (pos, d_nrm, d_tan), "not a torch tensor"), ("arity", (d_pos,), "needs")]
        for name, data, pattern in wrong:
            with pytest.raises(pt.PtrError, match="set_mesh_vertices_device: .*" + pattern):
                dev.set_mesh_vertices_device({0: data})
        same_arrays(dev.arrays(), before, "after what the wrapper refused")
        # and the call still works
        dev.set_mesh_vertices_device({0: (d_pos, None, d_tan)})
    finally:
        dev.close()
    # a scene without the flag, and one whose mesh was uploaded without tangents
    host = hosts("A")
    dev = upload(host, vertex_normals=False)
    try:
        before = dev.arrays()
        pos, nrm = dsc.original(host, 0)
        d_pos, d_nrm = on_device(pos), on_device(nrm)
        with pytest.raises(pt.PtrError, match="ptr_scene_set_mesh_vertices_device: mesh 0 has null normals .*PTR_DYNAMIC_VERTEX_NORMALS"):
            dev.set_mesh_vertices_device({0: (d_pos, None)})
        with pytest.raises(pt.PtrError, match="ptr_scene_set_mesh_vertices_device: .*without tangents"):
            dev.set_mesh_vertices_device({0: (d_pos, d_nrm, torch.ones((len(pos), 4), device="cuda"))})
        same_arrays(dev.arrays(), before, "after the refused calls on scene A")
    finally:
        dev.close()
    plain = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True)
    try:
        with pytest.raises(pt.PtrError, match="ptr_scene_set_mesh_vertices_device: the scene is not deformable"):
            plain.set_mesh_vertices_device({0: (d_pos, d_nrm)})
    finally:
        plain.close()


def test_memory_of_a_second_device_is_refused(hosts):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: there is no second device's memory to refuse")
    host = hosts("F-triangle")
    dev = upload(host)
    try:
        before = dev.arrays()
        pos, nrm = dsc.original(host, 0)
        far = torch.from_numpy(pos).to("cuda:1")
        rc, message = raw_call(dev, [(0, len(pos), far.data_ptr(), on_device(nrm).data_ptr(), 0)])
        assert rc != 0 and re.search("position array of mesh 0 is memory of device 1, not of the scene's device 0", message), message
        with pytest.raises(pt.PtrError, match="are on cuda:1, not on device 0"):
            dev.set_mesh_vertices_device({0: (far, on_device(nrm))})
        same_arrays(dev.arrays(), before, "after the refused call")
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 8. streams
def test_a_call_on_a_torch_stream_behind_its_producer(hosts):
    host = hosts("strip257")
    base = host.positions
    step = (dds.moved(base, seed=77) - base).astype(np.float32)
    pos = (base + step).astype(np.float32)   # what the producer computes: one float32 add per component
    dev, twin = upload(host), upload(host, vertex_normals=False)
    try:
        d_base, d_step = on_device(base), on_device(step)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d_pos = d_base + d_step          # enqueued on `stream`; the call reads it there (stream=None: torch's current stream)
            dev.set_mesh_vertices_device({0: (d_pos, None)})
        assert np.array_equal(d_pos.cpu().numpy().view(np.uint32), pos.view(np.uint32))
        twin.set_mesh_vertices({0: (pos, ref.normals(pos, host.indices))})
        same_arrays(dev.arrays(), twin.arrays(), "a call on torch's current stream")
        with torch.cuda.stream(stream):
            d_back = d_pos - d_step
        dev.set_mesh_vertices_device({0: (d_back, None)}, stream=stream.cuda_stream)
        back = (pos - step).astype(np.float32)
        twin.set_mesh_vertices({0: (back, ref.normals(back, host.indices))})
        same_arrays(dev.arrays(), twin.arrays(), "a call on a stream handle")
    finally:
        dev.close()
        twin.close()


# --------------------------------------------------------------------------------------------------------------------- 9. the old flags
def test_old_flags_upload_the_same_scene_through_either_call(hosts):
    host = hosts("A")
    lib = pt.load_library()
    err = C.create_string_buffer(512)
    old = pt.DeviceScene(host.desc, 0, keepalive=host, dynamic=True, deformable=True, primitives=True)
    new = object.__new__(pt.DeviceScene)
    new._h, new._keepalive, new._device = C.c_void_p(), host, 0
    assert lib.ptr_scene_upload_deformable(C.byref(host.desc), 0, 3, C.byref(new._h), err, len(err)) == 0, err.value
    try:
        assert old.dynamic_flags == new.dynamic_flags == 3
        a, b = old.arrays(), new.arrays()
        assert set(a) == set(b) == set(pt.SCENE_ARRAYS)
        for name in a:
            assert a[name].shape == b[name].shape and hashlib.sha256(a[name].tobytes()).hexdigest() == hashlib.sha256(b[name].tobytes()).hexdigest(), name
        s = small_settings(host)
        assert np.array_equal(old.render_image(s, 4)[0], new.render_image(s, 4)[0])
    finally:
        old.close()
        new.close()
