"""CPU tests of the surface of dynamic scenes on several devices (include/ptr_multi_dynamic.h): the exported functions and their ctypes
table, PtrMultiUpdateInfo against a compiled program, and every refusal that happens before device work.

A frame is created on devices only.  What is refused before a frame is looked at is called with a made-up handle that must never be
looked behind; what is refused against the frame's records - an index out of range or named twice, a non-finite or singular matrix,
the flags the frame was made with - goes through ptr_multi_frame_debug_check_update, which runs the calls' own check on records made
from the description on the host.  src_device at or past the visible count and a static frame need devices: tests/test_gpu_multi_dynamic.py."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import deform_scenes as dsc
import traversal_scenes as ts

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = {"ptr_multi_frame_create_dynamic": ("int", 7), "ptr_multi_frame_debug_create_dynamic_on": ("int", 8), "ptr_multi_frame_is_dynamic": ("int", 1),
          "ptr_multi_frame_dynamic_flags": ("uint32_t", 1), "ptr_multi_frame_set_mesh_transforms": ("int", 6),
          "ptr_multi_frame_set_mesh_vertices": ("int", 6), "ptr_multi_frame_set_spheres": ("int", 6), "ptr_multi_frame_set_rects": ("int", 6),
          "ptr_multi_frame_set_mesh_vertices_device": ("int", 8), "ptr_multi_frame_tree_cost": ("int", 4), "ptr_multi_frame_rebuild_tree": ("int", 5),
          "ptr_multi_frame_part_scene": ("PtrDeviceScene*", 2), "ptr_multi_frame_debug_check_update": ("int", 7)}
FRAME = C.c_void_p(0x1000)


def test_library_exports_every_function_of_the_header():
    text = open(os.path.join(ROOT, "include", "ptr_multi_dynamic.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {}
    for ret, name, args in re.findall(r"\b(int|uint32_t|PtrDeviceScene\*)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text):
        found[name] = (ret, args.count(",") + 1)
    assert found == COUNTS and set(found) == set(pt.MULTI_DYNAMIC_SYMBOLS) and len(pt.MULTI_DYNAMIC_SYMBOLS) == 13
    lib = pt.load_library()
    restypes = {"int": C.c_int, "uint32_t": C.c_uint32, "PtrDeviceScene*": C.c_void_p}
    for name, (ret, count) in found.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count and fn.restype is restypes[ret], name
    others = [pt.ABI_SYMBOLS, pt.DEBUG_SYMBOLS, pt.POST_SYMBOLS, pt.STATS_SYMBOLS, pt.ADAPTIVE_SYMBOLS, pt.MULTI_SYMBOLS, pt.FRAME_SYMBOLS,
              pt.MULTI_FRAME_SYMBOLS, pt.DYNAMIC_SYMBOLS, pt.DEFORM_SYMBOLS, pt.DEFORM_DEVICE_SYMBOLS, pt.BACKGROUND_SYMBOLS, pt.REBUILD_SYMBOLS]
    assert not set(pt.MULTI_DYNAMIC_SYMBOLS) & set().union(*map(set, others))
    assert len(pt.MULTI_FRAME_SYMBOLS) == 12, "the static frame's surface is what it was"


def test_python_mirrors_device_scene():
    for name in ("set_mesh_transforms", "set_mesh_vertices", "set_mesh_vertices_device", "set_spheres", "set_rects", "tree_cost", "rebuild_tree", "temporal"):
        assert callable(getattr(pt.MultiFrame, name)) and callable(getattr(pt.DeviceScene, name)), name
    assert callable(pt.MultiFrame.is_dynamic) and callable(pt.MultiFrame.part_scene)


def test_update_info_layout_against_a_compiled_program(tmp_path):
    fields = ["parts", "stagedParts", "totalSeconds", "distributeSeconds", "partSeconds", "first"]
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "ptr_multi_dynamic.h"\nint main() { std::printf("%zu %zu'
                   + " %zu" * len(fields) + '\\n", sizeof(PtrMultiUpdateInfo), sizeof(PtrUpdateInfo), '
                   + ", ".join("offsetof(PtrMultiUpdateInfo, %s)" % f for f in fields) + "); }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    info = pt.PtrMultiUpdateInfo
    assert [n for n, _ in info._fields_] == fields
    assert got == [C.sizeof(info), C.sizeof(pt.PtrUpdateInfo)] + [getattr(info, f).offset for f in fields]
    assert got[0] == 8 + 16 + 8 * pt.MULTI_MAX_PARTS + C.sizeof(pt.PtrUpdateInfo)
    # the header's struct names the same members in the same order
    text = open(os.path.join(ROOT, "include", "ptr_multi_dynamic.h")).read()
    body = re.search(r"typedef struct PtrMultiUpdateInfo \{(.*?)\} PtrMultiUpdateInfo;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\w+\])?;", body) == fields


def _call(name, *args):
    err = C.create_string_buffer(256)
    rc = getattr(pt.load_library(), name)(*args, err, len(err))
    return rc, err.value.decode()


def _refused(name, *args, words=None):
    rc, message = _call(name, *args)
    assert rc == 1 and message.startswith(name + ":") and (words is None or words in message), (name, rc, message)
    return message


def _settings(width=8, height=8):
    s = pt.PtrSettings()
    s.width, s.height, s.maxDepth = width, height, 2
    return s


def test_what_is_refused_before_a_frame_is_looked_at():
    one_t, one_v, one_d = (pt.PtrMeshTransform * 1)(), (pt.PtrMeshVertices * 1)(), (pt.PtrMeshVerticesDevice * 1)()
    one_s, one_r = (pt.PtrSphereUpdate * 1)(), (pt.PtrRectUpdate * 1)()
    info = pt.PtrMultiUpdateInfo()
    info.parts = 77
    for name, items, null_words in (("ptr_multi_frame_set_mesh_transforms", one_t, "null transform list"), ("ptr_multi_frame_set_mesh_vertices", one_v, "null mesh list"),
                                    ("ptr_multi_frame_set_spheres", one_s, "null list"), ("ptr_multi_frame_set_rects", one_r, "null list")):
        _refused(name, None, items, 1, C.byref(info), words="null argument")
        _refused(name, FRAME, None, 1, C.byref(info), words=null_words)
        _refused(name, FRAME, items, 0, C.byref(info), words="count is 0")
    name = "ptr_multi_frame_set_mesh_vertices_device"
    _refused(name, None, one_d, 1, 0, None, C.byref(info), words="null argument")
    _refused(name, FRAME, None, 1, 0, None, C.byref(info), words="null mesh list")
    _refused(name, FRAME, one_d, 0, 0, None, C.byref(info), words="count is 0")
    _refused(name, FRAME, one_d, 1, -1, None, C.byref(info), words="no such HIP device")
    assert info.parts == 77, "a refused call leaves the info alone"
    cost = C.c_double(7.0)
    _refused("ptr_multi_frame_tree_cost", None, C.byref(cost), words="null argument")
    _refused("ptr_multi_frame_tree_cost", FRAME, None, words="null argument")
    rebuild = pt.PtrRebuildInfo()
    _refused("ptr_multi_frame_rebuild_tree", None, 0, C.byref(rebuild), words="null argument")
    for flags in (2, 6, 0x80000001):
        _refused("ptr_multi_frame_rebuild_tree", FRAME, flags, C.byref(rebuild), words="unknown flag bits")
    assert cost.value == 7.0
    lib = pt.load_library()
    assert lib.ptr_multi_frame_is_dynamic(None) == 0 and lib.ptr_multi_frame_dynamic_flags(None) == 0
    assert lib.ptr_multi_frame_part_scene(None, 0) is None


def test_what_the_checks_against_the_frames_records_refuse():
    """Step 1 of every update call on records made from scene A (one mesh without tangents, a sphere, rectangles of which 5 is the light)."""
    host = ts.scene_a()
    desc, meshes, spheres, rects = host.desc, host.desc.meshCount, host.desc.sphereCount, host.desc.rectCount
    pos, nrm, _, _ = dsc.mesh_data(host)
    nan_matrix = np.eye(4, dtype=np.float32)
    nan_matrix[2, 1] = np.nan
    nan_pos = pos.copy()
    nan_pos[len(pos) // 2, 2] = np.inf
    light = dsc.rect_of(host, 5)
    check = pt.debug_multi_check_update
    # what is accepted goes on to the devices
    for call, update in (("set_mesh_transforms", {0: np.eye(4)}), ("set_mesh_vertices", {0: (pos, nrm)}), ("set_spheres", {0: (1.0, 2.0, 3.0, 4.0)}),
                         ("set_rects", {5: light})):
        check(desc, call, update)
    refused = [("set_mesh_transforms", {meshes: np.eye(4)}, "mesh index %d out of range \\(the scene has %d meshes\\)" % (meshes, meshes)),
               ("set_mesh_transforms", {0: nan_matrix}, "the matrix of mesh 0 has a non-finite entry"),
               ("set_mesh_transforms", {0: np.diag([2.0, 0.0, 1.0, 1.0])}, "the matrix of mesh 0 has a zero 3x3 determinant"),
               ("set_mesh_vertices", {meshes + 3: (pos, nrm)}, "mesh index %d out of range" % (meshes + 3)),
               ("set_mesh_vertices", {0: (pos[:-1], nrm[:-1])}, "mesh 0 was uploaded with %d vertices, not vertexCount %d" % (len(pos), len(pos) - 1)),
               ("set_mesh_vertices", {0: (pos, nrm, np.ones((len(pos), 4), np.float32))}, "mesh 0 was uploaded without tangents and is given some"),
               ("set_mesh_vertices", {0: (nan_pos, nrm)}, "mesh 0 has a non-finite position component"),
               ("set_spheres", {spheres: (0.0, 0.0, 0.0, 1.0)}, "sphere index %d out of range" % spheres),
               ("set_spheres", {0: (0.0, np.nan, 0.0, 1.0)}, "sphere 0 has a non-finite entry"),
               ("set_rects", {rects: light}, "rectangle index %d out of range" % rects),
               ("set_rects", {5: dict(light, edgeV=light["edgeU"])}, "rectangle 5 has cross\\(edgeU, edgeV\\) of length zero")]
    for call, update, words in refused:
        with pytest.raises(pt.PtrError, match="^ptr_multi_frame_%s: %s" % (call, words)):
            check(desc, call, update)
    # an index named twice cannot be said with a dict: through the C interface
    lib, err = pt.load_library(), C.create_string_buffer(256)
    twice = (pt.PtrMeshTransform * 2)()
    for item in twice:
        item.localToWorld[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
    assert lib.ptr_multi_frame_debug_check_update(C.byref(desc), 3, 0, twice, 2, err, len(err)) == 1
    assert err.value == b"ptr_multi_frame_set_mesh_transforms: mesh index 0 named twice"
    both = (pt.PtrSphereUpdate * 2)()
    assert lib.ptr_multi_frame_debug_check_update(C.byref(desc), 3, 2, both, 2, err, len(err)) == 1
    assert err.value == b"ptr_multi_frame_set_spheres: sphere index 0 named twice"
    # the flags the frame was made with, in the single-device words
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_set_mesh_vertices: the scene is not deformable \\(upload it with ptr_scene_upload_dynamic_ex"):
        check(desc, "set_mesh_vertices", {0: (pos, nrm)}, deformable=False)
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_set_rects: the scene does not keep its primitives"):
        check(desc, "set_rects", {5: light}, primitives=False)
    check(desc, "set_mesh_transforms", {0: np.eye(4)}, deformable=False, primitives=False)   # flags 0: ptr_scene_upload_dynamic
    # ... and the probe's own arguments
    for args, words in (((None, 3, 0, twice, 1), "null argument"), ((C.byref(desc), 3, 4, twice, 1), "no such kind"), ((C.byref(desc), 8, 0, twice, 1), "unknown flag"),
                        ((C.byref(desc), 3, 0, None, 1), "ptr_multi_frame_set_mesh_transforms: null transform list"),
                        ((C.byref(desc), 3, 0, twice, 0), "ptr_multi_frame_set_mesh_transforms: count is 0")):
        assert lib.ptr_multi_frame_debug_check_update(*args, err, len(err)) == 1 and words in err.value.decode(), (words, err.value)


def test_what_the_create_calls_refuse():
    desc, good, out = C.byref(pt.PtrSceneDesc()), _settings(), C.c_void_p()
    ids = (C.c_int * 2)(0, 0)
    # the flag rules of the uploads, in their words
    for flags, words in ((8, "unknown flag"), (15, "unknown flag"), (4, "PTR_DYNAMIC_VERTEX_NORMALS needs PTR_DYNAMIC_DEFORMABLE"),
                         (6, "PTR_DYNAMIC_VERTEX_NORMALS needs PTR_DYNAMIC_DEFORMABLE")):
        assert _refused("ptr_multi_frame_create_dynamic", desc, C.byref(good), 1, flags, C.byref(out)).endswith(": " + words)
        assert _refused("ptr_multi_frame_debug_create_dynamic_on", desc, C.byref(good), flags, ids, 2, C.byref(out)).endswith(": " + words)
    err = C.create_string_buffer(256)
    assert pt.load_library().ptr_scene_upload_deformable(desc, 0, 4, C.byref(out), err, len(err)) == 1
    assert err.value.decode().split(": ", 1)[1] == "PTR_DYNAMIC_VERTEX_NORMALS needs PTR_DYNAMIC_DEFORMABLE"
    # ... and those of ptr_multi_frame_create
    for args in ((None, C.byref(good), 1, 3, C.byref(out)), (desc, None, 1, 3, C.byref(out)), (desc, C.byref(good), 1, 3, None),
                 (desc, C.byref(_settings(0, 8)), 1, 3, C.byref(out)), (desc, C.byref(good), 65, 3, C.byref(out))):
        _refused("ptr_multi_frame_create_dynamic", *args)
    for args in ((None, C.byref(good), 3, ids, 2, C.byref(out)), (desc, C.byref(good), 3, None, 2, C.byref(out)), (desc, C.byref(good), 3, ids, 0, C.byref(out)),
                 (desc, C.byref(good), 3, (C.c_int * 65)(), 65, C.byref(out))):
        _refused("ptr_multi_frame_debug_create_dynamic_on", *args)
    assert not out.value
    with pytest.raises(pt.PtrError, match="need dynamic=True"):
        pt.multi_frame(pt.PtrSceneDesc(), good, device_ids=[0], deformable=True)


def test_dynamic_frames_fail_loudly_without_gpu():
    if pt.device_count() > 0:
        pytest.skip("a GPU is present")
    desc, good, out = C.byref(pt.PtrSceneDesc()), _settings(), C.c_void_p()
    for flags in (0, 1, 3, 5, 7):
        for name, args in (("ptr_multi_frame_create_dynamic", (desc, C.byref(good), 0, flags, C.byref(out))),
                           ("ptr_multi_frame_debug_create_dynamic_on", (desc, C.byref(good), flags, (C.c_int * 2)(0, 0), 2, C.byref(out)))):
            rc, message = _call(name, *args)
            assert rc == 2 and message.startswith(name + ":") and "no CPU fallback" in message and not out.value, (name, flags)
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.multi_frame(pt.PtrSceneDesc(), good, device_ids=[0, 0], dynamic=True, deformable=True)
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.multi_frame(pt.PtrSceneDesc(), good, dynamic=True)
